"""ctypes binding of libkpdi.so (include/kpdi.h) - no PyTorch, no NumPy C-API.

The library is built in-tree by `make -C kikuchipy_amd/csrc` (or
`__graft_entry__.build()`).  There is no CPU fallback anywhere in this
package: if the library is missing, or no gfx950 GPU is visible, calls raise.
"""

import atexit
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KPDI_LIB_PATH: another build of the library (kernel experiments, tools/README.md)
LIB_PATH = os.environ.get("KPDI_LIB_PATH") or os.path.join(_HERE, "csrc", "libkpdi.so")

METRIC_NCC, METRIC_NDP = 0, 1
COMPUTE_F32, COMPUTE_F16X2, COMPUTE_F16, COMPUTE_F64 = 0, 1, 2, 3
GATHER_AUTO, GATHER_RCCL, GATHER_P2P, GATHER_NONE = 0, 1, 2, 3
GATHER_NAMES = {GATHER_RCCL: "rccl", GATHER_P2P: "p2p", GATHER_NONE: "none"}
F64_CERTIFICATES = {0: None, 1: "statistical", 2: "worstcase"}
OP_SUBTRACT, OP_DIVIDE = 0, 1
DOMAIN_FREQUENCY, DOMAIN_SPATIAL = 0, 1
CENTRE_NONE, CENTRE_NAVIGATION, CENTRE_SIGNAL = 0, 1, 2  # kpdi_decomposition_*: what centring subtracts
DECOMPOSITION_MAX_SIDE = 8192  # csrc/decomp_plan.h, DEC_MAX_SIDE
HEMISPHERE_CODES = {"upper": 0, "lower": 1, "both": 2}  # kpdi_kinematical_master_pattern
KINEMATICAL_MAX_HALF_SIZE = 4096  # csrc/kinematical_plan.h, KIN_MAX_HALF_SIZE
SAMPLING_MAX_STEPS, SAMPLING_MAX_FACES = 2048, 23  # csrc/sampling_plan.h, SMP_MAX_STEPS and SMP_MAX_FACES
ORIENTATION_MAX_OPS, ORIENTATION_MAX_DIMS, ORIENTATION_MAX_OFFSETS = 24, 8, 1024  # csrc/orientations_plan.h, ORI_MAX_*
GEOMETRICAL_LINES, GEOMETRICAL_ZONE_AXES = 0, 1  # kpdi_geometrical_visibility
GEOMETRICAL_UPPER, GEOMETRICAL_INSIDE = 1, 2     # bits of its flags
GEOMETRICAL_PC_DOUBLES = 8  # csrc/geometrical_plan.h, GEO_PC_DOUBLES
UNIQUE_ID_BYTES = 128
REFINE_ORI, REFINE_PC, REFINE_ORI_PC = 0, 1, 2
REFINE_SIZES = {REFINE_ORI: (3, 3), REFINE_PC: (3, 4), REFINE_ORI_PC: (6, 0)}  # (control variables, fixed values)
REFINE_RESULT_STRIDE = 9

DTYPE_CODES = {
    np.dtype(np.uint8): 0,
    np.dtype(np.uint16): 1,
    np.dtype(np.float32): 2,
    np.dtype(np.float64): 3,
    np.dtype(np.int8): 4,
    np.dtype(np.int16): 5,
    np.dtype(np.int32): 6,
    np.dtype(np.uint32): 7,
    np.dtype(np.float16): 8,
}


class KpdiError(RuntimeError):
    """A libkpdi call failed (message from kpdi_last_error())."""


class KpdiIOError(KpdiError, OSError):
    """A file could not be read (`kikuchipy_amd.load`): an `OSError` like the reference's reader raises
    (io/plugins/_h5ebsd.py:210, :292-300), and a `KpdiError` like every failed libkpdi call."""


class Counters(C.Structure):
    _fields_ = [
        ("match_ms", C.c_double),
        ("match_launches", C.c_int64),
        ("match_flops", C.c_double),
        ("prep_ms", C.c_double),
        ("merge_ms", C.c_double),
        ("h2d_bytes", C.c_double),
        ("match_grid", C.c_int32),
        ("match_nsplit", C.c_int32),
        ("kpad", C.c_int32),
        ("k_kept", C.c_int32),
        ("project_ms", C.c_double),
        ("refine_ms", C.c_double),
        ("preproc_ms", C.c_double),
        ("preproc_launches", C.c_int64),
        ("rescore_ms", C.c_double),
        ("rescore_extra_passes", C.c_int64),
        ("uncertified_patterns", C.c_int64),
        ("match_form", C.c_int32),
        ("comm_ranks", C.c_int32),
        ("comm_ms", C.c_double),
        ("fixed_ms", C.c_double),
        ("f64_certificate", C.c_int32),
        ("gather_ranks", C.c_int32),
        ("coalesced_sweeps", C.c_int64),
        ("epi_lists", C.c_int64),
        ("epi_appended", C.c_int64),
        ("epi_overflows", C.c_int64),
        ("epi_direct_first", C.c_int64),
        ("kinematical_ms", C.c_double),
        ("geometrical_visibility_ms", C.c_double),
        ("geometrical_coordinates_ms", C.c_double),
        ("sampling_ms", C.c_double),
        ("orientation_ms", C.c_double),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class H5ebsdInfo(C.Structure):
    _fields_ = [
        ("scan", C.c_char * 64),
        ("ny", C.c_int32), ("nx", C.c_int32), ("sy", C.c_int32), ("sx", C.c_int32),
        ("dtype", C.c_int32),
        ("has_static_background", C.c_int32),
        ("static_background_dtype", C.c_int32),
        ("binning", C.c_int32),
        ("n_stored", C.c_int64),
        ("n_pc", C.c_int64),
        ("step_y", C.c_double), ("step_x", C.c_double), ("detector_pixel_size", C.c_double),
        ("sample_tilt", C.c_double), ("azimuth_angle", C.c_double), ("elevation_angle", C.c_double),
    ]


class PlanLaunch(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("row_first", "rows", "xcd_rows", "xcd_splits", "rows_grid")]


class Plan(C.Structure):
    """kpdi_plan (include/kpdi.h): what the launch planner decides for a sweep."""
    _fields_ = ([(n, C.c_int32) for n in ("form", "tile", "row_blocks", "n_tiles", "nsplit", "rows_per_launch", "launches")]
                + [("round_rows", C.c_int64)]
                + [(n, C.c_int32) for n in ("n_main", "tail_tiles", "tail_units", "tail_nsplit", "fixed_draws", "tail_first",
                                            "tail_shift", "perm_rounds", "perm_stride", "tail_gemm_rows", "n_launch_desc")]
                + [("launch", PlanLaunch * 64)])


# every symbol include/kpdi.h declares: (restype, argtypes)
_vp, _i, _i64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
SIGNATURES = {
    "kpdi_version": (C.c_char_p, []),
    "kpdi_device_count": (_i, []),
    "kpdi_last_error": (C.c_char_p, []),
    "kpdi_create": (_i, [_i, C.POINTER(_vp)]),
    "kpdi_destroy": (_i, [_vp]),
    "kpdi_synchronize": (_i, [_vp]),
    "kpdi_set_problem": (_i, [_vp, _i, _i, _vp, _i, _i, _i]),
    "kpdi_set_keep_n": (_i, [_vp, _i]),
    "kpdi_set_experimental": (_i, [_vp, _vp, _i, _i64, _vp]),
    "kpdi_set_experimental_dev": (_i, [_vp, _vp, _i, _i64, _vp]),
    "kpdi_n_experimental": (_i64, [_vp]),
    "kpdi_remove_static_background": (_i, [_vp, _vp, _i, _i]),
    "kpdi_remove_dynamic_background": (_i, [_vp, _i, _i, C.c_double, C.c_double]),
    "kpdi_get_experimental": (_i, [_vp, _vp]),
    "kpdi_image_quality": (_i, [_vp, _i, _vp, C.c_double, _vp]),
    "kpdi_region_sums": (_i, [_vp, _vp, _i, _vp]),
    "kpdi_reduce_experimental": (_i, [_vp, _i, _i, _i, _i, _vp, _sz]),
    "kpdi_reduce_plan_describe": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp]),
    "kpdi_fft_filter": (_i, [_vp, _i, _vp, _i, _i]),
    "kpdi_rescale_intensity": (_i, [_vp, _vp, _vp, C.c_double, C.c_double, _i]),
    "kpdi_normalize_intensity": (_i, [_vp, C.c_double, _i, _i]),
    "kpdi_intensity_range": (_i, [_vp, _vp]),
    "kpdi_adaptive_histogram_equalization": (_i, [_vp, _i, _i, _i, _i]),
    "kpdi_downsample": (_i, [_vp, _i, _i]),
    "kpdi_get_dynamic_background": (_i, [_vp, _i, C.c_double, C.c_double, _i, _vp]),
    "kpdi_decomposition_gram": (_i, [_vp, _i, _vp, _vp, C.POINTER(_i64), C.POINTER(_i)]),
    "kpdi_decomposition_apply": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "kpdi_decomposition_model": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i]),
    "kpdi_change_dtype": (_i, [_vp, _i]),
    "kpdi_select_patterns": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i]),
    "kpdi_set_navigation_mask": (_i, [_vp, _vp]),
    "kpdi_kinematical_master_pattern": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _vp]),
    "kpdi_sample_fundamental_count": (_i, [_vp, _i, _vp, _i, C.POINTER(_i64)]),
    "kpdi_sample_fundamental_fill": (_i, [_vp, _i, _vp, _i, _vp, _i64, C.POINTER(_i64)]),
    "kpdi_orientation_pairs": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "kpdi_orientation_outer": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _i, _vp, _i, _i, _i, _vp]),
    "kpdi_orientation_reduce": (_i, [_vp, _vp, _i64, _vp, _i, _vp, _vp]),
    "kpdi_orientation_kam": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp, C.c_double, _i, _vp]),
    "kpdi_hough_default_n_rho": (_i, [_i, _i]),
    "kpdi_hough_plan_describe": (_i, [_i, _i, _i, _i, _i64, _i64, _i64, _vp]),
    "kpdi_hough_bands": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "kpdi_hough_index": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _i, _i, _vp, _vp, _vp, _i, _i, _vp, C.c_double, _vp, _vp, _vp,
                              _vp]),
    "kpdi_hough_optimize_pc": (_i, [_vp, _vp, _i64, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, C.c_double, C.c_double,
                                    C.c_double, C.c_double, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "kpdi_geometrical_visibility": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "kpdi_geometrical_coordinates": (_i, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, C.c_double,
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    "kpdi_average_neighbour_patterns": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _i]),
    "kpdi_neighbour_dot_products": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "kpdi_push_dictionary_chunk": (_i, [_vp, _vp, _i, _i64, _i64]),
    "kpdi_push_dictionary_chunk_dev": (_i, [_vp, _vp, _i, _i64, _i64]),
    "kpdi_set_master_pattern": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "kpdi_set_detector": (_i, [_vp, _vp, C.c_double, _i, _i, _vp]),
    "kpdi_set_direction_cosines": (_i, [_vp, _vp, _i64]),
    "kpdi_get_direction_cosines": (_i, [_vp, _vp]),
    "kpdi_project_patterns": (_i, [_vp, _vp, _i64, _i, C.c_double, C.c_double, _i, _vp]),
    "kpdi_project_patterns_varying_pc": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _i, C.c_double, C.c_double, _i, _vp]),
    "kpdi_push_rotations_chunk": (_i, [_vp, _vp, _i64, _i64, _i, C.c_double, C.c_double]),
    "kpdi_push_rotations_chunk_varying_pc": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _i, C.c_double, C.c_double]),
    "kpdi_hold_dictionary_chunk": (_i, [_vp, _vp, _i, _i64, _i64]),
    "kpdi_hold_dictionary_chunk_dev": (_i, [_vp, _vp, _i, _i64, _i64]),
    "kpdi_hold_rotations_chunk": (_i, [_vp, _vp, _i64, _i64, _i, C.c_double, C.c_double]),
    "kpdi_sweep_held": (_i, [_vp]),
    "kpdi_release_held": (_i, [_vp]),
    "kpdi_held_size": (_i, [_vp, _vp, _vp]),
    "kpdi_refine_set_patterns": (_i, [_vp, _vp, _i, _i64, _i, _i, _vp, _i, _vp]),
    "kpdi_refine_get_prepared": (_i, [_vp, _vp, _vp]),
    "kpdi_refine_objective": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp]),
    "kpdi_refine_solve": (_i, [_vp, _i, _i64, _i, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i, _i, _vp]),
    "kpdi_nelder_mead_selftest": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_double, C.c_double, _i, _i, _vp]),
    "kpdi_refine_solve_powell": (_i, [_vp, _i, _i64, _i, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i, _i, _vp, _i64, _vp,
                                      _i]),
    "kpdi_powell_selftest": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.c_double, C.c_double, _i, _i, _vp]),
    "kpdi_refine_solve_nlopt": (_i, [_vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, _i, _vp]),
    "kpdi_nlopt_simplex_selftest": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, C.c_double, _i, _vp]),
    "kpdi_refine_solve_de": (_i, [_vp, _i, _i64, _i, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, C.c_double, C.c_double,
                                  C.c_double, _i, _i, _vp, _vp, _i64, _vp, _i]),
    "kpdi_de_selftest": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                              _i, _i, C.c_uint32, _vp]),
    "kpdi_refine_solve_basinhopping": (_i, [_vp, _i, _i64, _i, _vp, _vp, _i, C.c_double, C.c_double, _i, _i, C.c_double,
                                            C.c_double, C.c_double, C.c_double, _i, _i, _vp, _vp, _i64, _vp, _i]),
    "kpdi_basinhopping_selftest": (_i, [_vp, _i, _i, _vp, _i, C.c_double, C.c_double, _i, _i, C.c_double, C.c_double,
                                        C.c_double, C.c_double, _i, _i, C.c_uint32, _vp]),
    "kpdi_mt19937_selftest": (_i, [_vp, C.c_uint32, _vp, _i, _vp, _i64]),
    "kpdi_merge_selftest": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, C.c_uint32,
                                 _vp, _vp, _i, _vp, _vp]),
    "kpdi_merge64_selftest": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i64, _i, _i, _i64, _i64, _vp, _i, _i, _i,
                                   C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "kpdi_rescore_selftest": (_i, [_vp, _vp, _i, _i64, _vp, _i, _vp, _i, _i64, _i64, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i,
                                   C.c_float, _vp, _vp, _vp]),
    "kpdi_fill_selftest": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i64]),
    "kpdi_orientation_similarity_map": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "kpdi_dtype_size": (_sz, [_i]),
    "kpdi_plan_describe": (_i, [_i64, _i64, _i, _i, _i, _i, C.POINTER(Plan)]),
    "kpdi_h5ebsd_info_read": (_i, [C.c_char_p, C.c_char_p, C.POINTER(H5ebsdInfo)]),
    "kpdi_h5ebsd_read_patterns": (_i, [C.c_char_p, C.c_char_p, _vp, _sz]),
    "kpdi_h5ebsd_read_static_background": (_i, [C.c_char_p, C.c_char_p, _vp, _sz]),
    "kpdi_h5ebsd_read_pc": (_i, [C.c_char_p, C.c_char_p, _vp, _i64]),
    "kpdi_set_experimental_h5ebsd": (_i, [_vp, C.c_char_p, C.c_char_p, _vp]),
    "kpdi_reset_topk": (_i, [_vp]),
    "kpdi_finalize": (_i, [_vp, _vp, _vp]),
    "kpdi_finalize_f64": (_i, [_vp, _vp, _vp]),
    "kpdi_finalize_async": (_i, [_vp, C.POINTER(_i)]),
    "kpdi_finalize_wait": (_i, [_vp, _i, _vp, _vp]),
    "kpdi_pending_result_size": (_i, [_vp, _i, C.POINTER(_i64)]),
    "kpdi_result_indices_i32": (_i, [_vp, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(_i64)]),
    "kpdi_comm_unique_id": (_i, [_vp]),
    "kpdi_comm_init": (_i, [_vp, _i, _i, _vp]),
    "kpdi_comm_selftest": (_i, [_vp, _i64, _i]),
    "kpdi_comm_drop": (_i, [_vp]),
    "kpdi_export_lists": (_i, [_vp, _vp, _vp]),
    "kpdi_import_lists": (_i, [_vp, _vp, _vp, _i]),
    "kpdi_dev_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "kpdi_dev_free": (_i, [_vp, _vp]),
    "kpdi_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "kpdi_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "kpdi_set_profiling": (_i, [_vp, _i]),
    "kpdi_get_counters": (_i, [_vp, C.POINTER(Counters)]),
    "kpdi_reset_counters": (_i, [_vp]),
    "kpdi_counters_size": (_sz, []),
    # a group of contexts: several GPUs from one thread of one process
    "kpdi_group_create": (_i, [C.POINTER(_i), _i, _i, C.POINTER(_vp)]),
    "kpdi_group_destroy": (_i, [_vp]),
    "kpdi_group_size": (_i, [_vp]),
    "kpdi_group_gather": (_i, [_vp]),
    "kpdi_group_describe": (C.c_char_p, [_vp]),
    "kpdi_group_member": (_vp, [_vp, _i]),
    "kpdi_group_chunk_share": (_i, [_i64, _i, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "kpdi_group_assign_chunk": (_i, [_i, _i64, _i64, C.POINTER(_i64), _i64, _i, C.POINTER(_i), C.POINTER(_i64),
                                     C.POINTER(_i64), C.POINTER(_i)]),
    "kpdi_group_set_dictionary_size": (_i, [_vp, _i64]),
    "kpdi_group_push_dictionary_chunk_borrowed": (_i, [_vp, _vp, _i, _i64, _i64, C.POINTER(_i64)]),
    "kpdi_group_chunks_consumed": (_i, [_vp, C.POINTER(_i64)]),
    "kpdi_group_synchronize": (_i, [_vp]),
    "kpdi_group_set_problem": (_i, [_vp, _i, _i, _vp, _i, _i, _i]),
    "kpdi_group_set_keep_n": (_i, [_vp, _i]),
    "kpdi_group_set_experimental": (_i, [_vp, _vp, _i, _i64, _vp]),
    "kpdi_group_set_experimental_dev": (_i, [_vp, C.POINTER(_vp), _i, _i64, _vp]),
    "kpdi_group_n_experimental": (_i64, [_vp]),
    "kpdi_group_remove_static_background": (_i, [_vp, _vp, _i, _i]),
    "kpdi_group_remove_dynamic_background": (_i, [_vp, _i, _i, C.c_double, C.c_double]),
    "kpdi_group_get_experimental": (_i, [_vp, _vp]),
    "kpdi_group_push_dictionary_chunk": (_i, [_vp, _vp, _i, _i64, _i64]),
    "kpdi_group_push_dictionary_chunk_dev": (_i, [_vp, C.POINTER(_vp), _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "kpdi_group_set_master_pattern": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "kpdi_group_set_detector": (_i, [_vp, _vp, C.c_double, _i, _i, _vp]),
    "kpdi_group_push_rotations_chunk": (_i, [_vp, _vp, _i64, _i64, _i, C.c_double, C.c_double]),
    "kpdi_group_hold_dictionary_chunk": (_i, [_vp, _vp, _i, _i64, _i64]),
    "kpdi_group_hold_rotations_chunk": (_i, [_vp, _vp, _i64, _i64, _i, C.c_double, C.c_double]),
    "kpdi_group_sweep_held": (_i, [_vp]),
    "kpdi_group_release_held": (_i, [_vp]),
    "kpdi_group_held_size": (_i, [_vp, _vp, _vp]),
    "kpdi_group_reset_topk": (_i, [_vp]),
    "kpdi_group_finalize": (_i, [_vp, _vp, _vp]),
    "kpdi_group_finalize_f64": (_i, [_vp, _vp, _vp]),
    "kpdi_group_finalize_async": (_i, [_vp, C.POINTER(_i)]),
    "kpdi_group_finalize_wait": (_i, [_vp, _i, _vp, _vp]),
    "kpdi_group_pending_result_size": (_i, [_vp, _i, C.POINTER(_i64)]),
    "kpdi_group_set_profiling": (_i, [_vp, _i]),
    "kpdi_group_reset_counters": (_i, [_vp]),
}

_lib = None


def load():
    """Load libkpdi.so once; raise (never fall back) when it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise KpdiError(
                f"{LIB_PATH} not found: build it with `make -C kikuchipy_amd/csrc` "
                "(python -c 'import __graft_entry__ as g; g.build()'). kikuchipy_amd has no "
                "CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        # kpdi_counters has grown between versions: a stale struct here would be written past its end
        if lib.kpdi_counters_size() != C.sizeof(Counters):
            raise KpdiError(f"{LIB_PATH} ({lib.kpdi_version().decode()}) was built with a kpdi_counters of "
                            f"{lib.kpdi_counters_size()} bytes, this binding expects {C.sizeof(Counters)}: rebuild "
                            "the library (make -C kikuchipy_amd/csrc)")
        _lib = lib
    return _lib


def last_error():
    return (load().kpdi_last_error() or b"").decode()


def check(rc):
    if rc != 0:
        raise KpdiError(f"libkpdi error {rc}: {last_error()}")


def device_count():
    return int(load().kpdi_device_count())


def version():
    return load().kpdi_version().decode()


def plan_describe(m, n_chunk, k_kept=3600, keep_n=20, n_cu=256, form=-1):
    """The launch plan of a sweep (csrc/plan.h) as a `Plan`; host arithmetic, needs no GPU."""
    p = Plan()
    check(load().kpdi_plan_describe(int(m), int(n_chunk), int(k_kept), int(keep_n), int(n_cu), int(form), C.byref(p)))
    return p


def dtype_code(dtype):
    try:
        return DTYPE_CODES[np.dtype(dtype)]
    except KeyError:
        raise KpdiError(f"pattern dtype {np.dtype(dtype)} is not supported by libkpdi") from None


DTYPE_FROM_CODE = {code: dt for dt, code in DTYPE_CODES.items()}

REDUCE_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3, "std": 4, "var": 5}  # KPDI_REDUCE_*
REDUCE_PLAN_FIELDS = ("regime", "A", "R1", "M", "R2", "B", "slice", "n_slices", "vec", "group", "grid_x", "grid_y", "passes",
                      "planes", "workspace_bytes", "result_bytes", "combine_lanes")
REDUCE_COLS, REDUCE_RUNS = 0, 1  # csrc/reduce_plan.h: the inner axis survives / contiguous runs are reduced
REDUCE_COLS_SLICE, REDUCE_RUNS_VECS, REDUCE_THREADS = 128, 16, 256  # RED_COLS_SLICE, RED_RUNS_VECS, RED_THREADS
REDUCE_COMBINE_SERIAL, REDUCE_COMBINE_LANES = 32, 16  # RED_COMBINE_SERIAL, RED_COMBINE_LANES


def reduce_dtype(dtype, op):
    """NumPy's result dtype of `op` over patterns of `dtype` (checked under NumPy 2.2.6): sum -> uint64 / int64 / the
    float dtype; mean, std, var -> float64 / the float dtype; max, min -> the dtype."""
    dtype = np.dtype(dtype)
    if op not in REDUCE_OPS:
        raise ValueError(f"op {op!r} must be one of {list(REDUCE_OPS)}")
    if dtype.kind == "f" or op in ("max", "min"):
        return dtype
    if op == "sum":
        return np.dtype(np.uint64 if dtype.kind == "u" else np.int64)
    return np.dtype(np.float64)


def reduce_plan_describe(dtype, op, axis_mask, ny, nx, sy, sx):
    """The plan of a `Context.reduce` (csrc/reduce_plan.h) as a dict of `REDUCE_PLAN_FIELDS`; host arithmetic, needs no
    GPU.  `axis_mask`: bit k = axis k of (ny, nx, sy, sx) is reduced."""
    desc = (C.c_int64 * len(REDUCE_PLAN_FIELDS))()
    check(load().kpdi_reduce_plan_describe(dtype_code(dtype), REDUCE_OPS[op], int(axis_mask), int(ny), int(nx), int(sy),
                                           int(sx), desc))
    return dict(zip(REDUCE_PLAN_FIELDS, (int(v) for v in desc)))


# csrc/hough_plan.h: one detected band (HoughBand), the limits, and what kpdi_hough_plan_describe fills in
HOUGH_BAND_DTYPE = np.dtype([("theta", "<f4"), ("rho", "<f4"), ("value", "<f4"), ("valid", "<i4"), ("a", "<i4"), ("k", "<i4"),
                             ("da", "<f4"), ("dk", "<f4")])
HOUGH_MAX_BANDS, HOUGH_MAX_REFLECTORS, HOUGH_MAX_FAMILIES = 16, 96, 16
HOUGH_SEARCH_MAX_EVALS = 10000  # csrc/hough_plan.h: a budget that allows one search more evaluations is refused by the kernel call
HOUGH_SEARCH_EVALS = 6  # csrc/hough_plan.h: evaluations per lane and launch of the projection-centre search by default
HOUGH_PLAN_FIELDS = ("ok", "lds", "lds_bytes", "pattern_bytes", "pass_patterns", "n_passes", "tail_patterns")


def hough_default_n_rho(ny, nx):
    """One pixel per rho cell over the inscribed circle (csrc/hough_plan.h)."""
    return int(load().kpdi_hough_default_n_rho(int(ny), int(nx)))


def hough_plan_describe(ny, nx, n_theta, n_rho, m, room_bytes, forced=0):
    """The launch plan of `Context.hough_bands` (csrc/hough_plan.h) as a dict of `HOUGH_PLAN_FIELDS`; host arithmetic."""
    desc = (C.c_int64 * len(HOUGH_PLAN_FIELDS))()
    check(load().kpdi_hough_plan_describe(int(ny), int(nx), int(n_theta), int(n_rho), int(m), int(room_bytes), int(forced), desc))
    return dict(zip(HOUGH_PLAN_FIELDS, (int(v) for v in desc)))


def _cstr(s):
    return None if s is None else os.fsencode(s)


def h5ebsd_info(path, scan=None):
    info = H5ebsdInfo()
    check(load().kpdi_h5ebsd_info_read(_cstr(path), _cstr(scan), C.byref(info)))
    return info


def h5ebsd_read(path, scan=None):
    """(info, patterns (ny, nx, sy, sx), static background or None, PCs (n_pc, 3) or None)."""
    info = h5ebsd_info(path, scan)
    name = info.scan
    pats = np.empty((info.ny, info.nx, info.sy, info.sx), dtype=DTYPE_FROM_CODE[info.dtype])
    check(load().kpdi_h5ebsd_read_patterns(_cstr(path), name, _ptr(pats), pats.nbytes))
    bg = None
    if info.has_static_background:
        bg = np.empty((info.sy, info.sx), dtype=DTYPE_FROM_CODE[info.static_background_dtype])
        check(load().kpdi_h5ebsd_read_static_background(_cstr(path), name, _ptr(bg), bg.nbytes))
    pc = None
    if info.n_pc > 0:
        pc = np.empty((info.n_pc, 3), dtype=np.float64)
        check(load().kpdi_h5ebsd_read_pc(_cstr(path), name, _ptr(pc), info.n_pc))
    return info, pats, bg, pc


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mask_bytes(mask):
    if mask is None:
        return None
    return np.ascontiguousarray(np.asarray(mask).ravel().astype(np.uint8))


class _Functions:
    """`f.set_problem` -> `libkpdi.kpdi_set_problem` (prefix "kpdi_") or `kpdi_group_set_problem`
    (prefix "kpdi_group_"): lets `Group` reuse `Context`'s methods for every call that has a group form.  A `Context`
    method without one is named in `Group._ON_ROOT` (runs on member 0) or `Group._ONE_GPU` (refused), or `Group`
    overrides it by hand; tests/test_host_group.py checks that every public method is one of the four."""

    def __init__(self, prefix):
        self._prefix = prefix

    def __getattr__(self, name):
        fn = getattr(load(), self._prefix + name)
        setattr(self, name, fn)
        return fn


class Context:
    """One GPU, one stream: thin object wrapper over a `kpdi_ctx*`."""

    _prefix = "kpdi_"

    def __init__(self, device=0, _borrowed=None):
        self._f = _Functions(self._prefix)
        self._owned = _borrowed is None
        if _borrowed is not None:  # a member of a `Group`: the group owns the kpdi_ctx
            self._h = C.c_void_p(_borrowed)
        else:
            self._h = C.c_void_p()
            check(self._f.create(int(device), C.byref(self._h)))
        self.device = int(device)
        self._init_state()

    def _init_state(self):
        """The Python-side state of a fresh engine, `Context` or `Group` alike."""
        self._keep = {}  # host arrays the library may still be reading
        self._keep_n = None       # what kpdi_finalize will write per pattern
        self._compute = COMPUTE_F32
        self._projection_key = None  # simulations.ProjectedDictionary.configure
        self.result_token = 0     # bumped by every finalize()
        self._last_valid = False   # the last finalize() succeeded: its lists may still be resident in HBM
        self._host_gather = None   # a parallel.Communicator whose ranks gather their lists over the control plane

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if self._owned:
                self._f.destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        check(self._f.synchronize(self._h))

    # -- set-up
    def set_problem(self, sy, sx, signal_mask=None, metric=METRIC_NCC, keep_n=20, compute=COMPUTE_F32):
        sm = _mask_bytes(signal_mask)
        if sm is not None and sm.size != sy * sx:
            raise KpdiError(f"signal mask has {sm.size} elements, detector has {sy * sx}")
        check(self._f.set_problem(self._h, int(sy), int(sx), _ptr(sm), int(metric), int(compute),
                                      int(keep_n)))
        self._keep_n = int(keep_n)
        self._compute = int(compute)
        self._detector = (int(sy), int(sx))

    def set_keep_n(self, keep_n):
        check(self._f.set_keep_n(self._h, int(keep_n)))
        self._keep_n = int(keep_n)

    def set_experimental(self, patterns, navigation_mask=None):
        """patterns: (m_all, sy, sx) or (m_all, sy*sx), C-contiguous."""
        p = np.ascontiguousarray(patterns)
        nm = _mask_bytes(navigation_mask)
        m_all = p.shape[0]
        if nm is not None and nm.size != m_all:
            raise KpdiError(f"navigation mask has {nm.size} elements, there are {m_all} patterns")
        check(self._f.set_experimental(self._h, _ptr(p), dtype_code(p.dtype), m_all, _ptr(nm)))
        check(self._f.synchronize(self._h))  # upload done: `p` may be a temporary
        self._exp_shape, self._exp_dtype = p.shape, p.dtype

    def set_experimental_h5ebsd(self, path, scan=None, navigation_mask=None):
        """Patterns of a kikuchipy h5ebsd scan: file -> pinned host buffer -> HBM."""
        info = h5ebsd_info(path, scan)
        nm = _mask_bytes(navigation_mask)
        if nm is not None and nm.size != info.ny * info.nx:
            raise KpdiError(f"navigation mask has {nm.size} elements, the scan has {info.ny * info.nx} patterns")
        check(self._f.set_experimental_h5ebsd(self._h, _cstr(path), info.scan, _ptr(nm)))
        self._exp_shape = (info.ny * info.nx, info.sy, info.sx)
        self._exp_dtype = DTYPE_FROM_CODE[info.dtype]
        return info

    def set_experimental_dev(self, d_ptr, dtype, m_all, navigation_mask=None):
        nm = _mask_bytes(navigation_mask)
        check(self._f.set_experimental_dev(self._h, C.c_void_p(d_ptr), dtype_code(dtype), int(m_all),
                                               _ptr(nm)))
        self._record_experimental_dev(dtype, m_all)

    def _record_experimental_dev(self, dtype, m_all):
        """What `get_experimental` allocates after a `set_experimental_dev`."""
        self._exp_shape, self._exp_dtype = (int(m_all),) + getattr(self, "_detector", (-1,)), np.dtype(dtype)

    @property
    def n_experimental(self):
        return int(self._f.n_experimental(self._h))

    # -- pre-processing
    def remove_static_background(self, static_bg_f32, operation=OP_SUBTRACT, scale_bg=False):
        bg = np.ascontiguousarray(static_bg_f32, dtype=np.float32)
        check(self._f.remove_static_background(self._h, _ptr(bg), int(operation), int(bool(scale_bg))))

    def remove_dynamic_background(self, operation=OP_SUBTRACT, filter_domain=DOMAIN_FREQUENCY, std=0.0,
                                  truncate=4.0):
        check(self._f.remove_dynamic_background(self._h, int(operation), int(filter_domain),
                                                    float(std), float(truncate)))

    def get_experimental(self):
        out = np.empty(self._exp_shape, dtype=self._exp_dtype)
        check(self._f.get_experimental(self._h, _ptr(out)))
        return out

    def image_quality(self, normalize=True, frequency_vectors=None, inertia_max=0.0):
        """Q of every resident pattern (after the recorded background steps): float32 (m_all,).  `frequency_vectors`:
        (sy, sx) weights or None (the reference's default); `inertia_max` <= 0: derived from the weights."""
        w = None if frequency_vectors is None else np.ascontiguousarray(frequency_vectors, dtype=np.float64)
        if w is not None and w.shape != self._detector:
            raise KpdiError(f"frequency vectors of shape {w.shape}, patterns of shape {self._detector}")
        out = np.empty(self._exp_shape[0], dtype=np.float32)
        check(self._f.image_quality(self._h, int(bool(normalize)), _ptr(w), float(inertia_max), _ptr(out)))
        return out

    def region_sums(self, rects):
        """np.nansum of every resident pattern (after the recorded background steps) over each rectangle of `rects`,
        (n_rects, 4) of (row0, row1, col0, col1), half-open and inside the detector: (m_all, n_rects) of uint64 (uint8 /
        uint16 patterns), int64 (int8 / int16), float32 or float64 (include/kpdi.h, kpdi_region_sums)."""
        r = np.ascontiguousarray(rects, dtype=np.int32)
        if r.ndim != 2 or r.shape[1] != 4:
            raise KpdiError(f"rectangles of shape {r.shape}, not (n_rects, 4)")
        kind = self._exp_dtype.kind
        dt = self._exp_dtype if kind == "f" else np.dtype(np.uint64 if kind == "u" else np.int64)
        out = np.zeros((self._exp_shape[0], len(r)), dtype=dt)
        check(self._f.region_sums(self._h, _ptr(r), len(r), _ptr(out)))
        return out

    def reduce(self, op, axes, navigation_shape):
        """`op` ("sum", "mean", "max", "min", "std", "var") of the resident patterns (after the recorded background
        steps), taken as an array of `navigation_shape` + (sy, sx), over its `axes` (array axes, each once): the kept
        axes in order, of NumPy's result dtype (include/kpdi.h, kpdi_reduce_experimental)."""
        nav = tuple(int(n) for n in navigation_shape)
        if len(nav) > 2:
            raise KpdiError(f"navigation shape {nav}: at most two navigation axes")
        shape = nav + tuple(self._detector)
        reduced = {int(ax) for ax in axes}
        if not reduced or min(reduced) < 0 or max(reduced) >= len(shape):
            raise KpdiError(f"axes {sorted(reduced)} of an array of {len(shape)} axes")
        first = 2 - len(nav)  # the library's array is always (ny, nx, sy, sx)
        ny, nx = ((1,) * first + nav)
        out = np.empty([n for k, n in enumerate(shape) if k not in reduced], dtype=reduce_dtype(self._exp_dtype, op))
        check(self._f.reduce_experimental(self._h, REDUCE_OPS[op], sum(1 << (ax + first) for ax in reduced), ny, nx,
                                          _ptr(out), out.nbytes))
        return out

    def fft_filter(self, function_domain, table):
        """Filter every resident pattern in place (after the recorded background steps) and rescale it to its dtype's
        range.  DOMAIN_FREQUENCY: `table` is the folded half spectrum, complex (sy, sx // 2 + 1); DOMAIN_SPATIAL: a real
        (ty, tx) correlation kernel (include/kpdi.h, kpdi_fft_filter)."""
        if int(function_domain) == DOMAIN_FREQUENCY:
            t = np.ascontiguousarray(table, dtype=np.complex128)
            flat = t.view(np.float64)
        else:
            t = flat = np.ascontiguousarray(table, dtype=np.float64)
        if t.ndim != 2:
            raise KpdiError(f"filter table of shape {t.shape}")
        check(self._f.fft_filter(self._h, int(function_domain), _ptr(flat), int(t.shape[0]), int(t.shape[1])))

    def rescale_intensity(self, in_range=None, percentiles=None, omin=0.0, omax=1.0, dtype_out=None):
        """Rescale every resident pattern (after the recorded background steps) onto [omin, omax] from `in_range`,
        the per-pattern `percentiles` or the per-pattern min / max, into `dtype_out` (None: the patterns' dtype); the
        resident patterns take the new dtype (include/kpdi.h, kpdi_rescale_intensity)."""
        dt = self._exp_dtype if dtype_out is None else np.dtype(dtype_out)
        ir = None if in_range is None else np.ascontiguousarray(in_range, dtype=np.float64).reshape(2)
        pc = None if percentiles is None else np.ascontiguousarray(percentiles, dtype=np.float64).reshape(2)
        check(self._f.rescale_intensity(self._h, _ptr(ir), _ptr(pc), float(omin), float(omax), dtype_code(dt)))
        self._exp_dtype = dt

    def downsample(self, factor, dtype_out=None):
        """Bin every resident pattern (after the recorded background steps) by `factor` and rescale it to the range of
        `dtype_out` (None: the patterns' dtype); the resident patterns and the problem take the new detector shape and
        dtype (include/kpdi.h, kpdi_downsample)."""
        dt = self._exp_dtype if dtype_out is None else np.dtype(dtype_out)
        check(self._f.downsample(self._h, int(factor), dtype_code(dt)))
        sy, sx = self._detector
        self._detector = (sy // int(factor), sx // int(factor))
        self._exp_shape = (self._exp_shape[0],) + self._detector
        self._exp_dtype = dt

    def get_dynamic_background(self, filter_domain=DOMAIN_FREQUENCY, std=None, truncate=4.0, dtype_out=None):
        """The Gaussian-blurred image of every resident pattern (after the recorded background steps) as `dtype_out`
        (None: the patterns' dtype): (m_all, sy, sx); `std` None: sx / 8 (include/kpdi.h,
        kpdi_get_dynamic_background).  The resident patterns stay as they are."""
        dt = self._exp_dtype if dtype_out is None else np.dtype(dtype_out)
        out = np.empty((self._exp_shape[0],) + self._detector, dtype=dt)
        check(self._f.get_dynamic_background(self._h, int(filter_domain), 0.0 if std is None else float(std),
                                             float(truncate), dtype_code(dt), _ptr(out)))
        return out

    def change_dtype(self, dtype_out):
        """`ndarray.astype(dtype_out)` of the resident patterns (after the recorded background steps), which take the
        new dtype (include/kpdi.h, kpdi_change_dtype)."""
        dt = np.dtype(dtype_out)
        check(self._f.change_dtype(self._h, dtype_code(dt)))
        self._exp_dtype = dt

    def select_patterns(self, pattern_index=None, rows=None, cols=None, into=None):
        """out[i, r, c] = in[pattern_index[i], rows[r], cols[c]] of the resident patterns (after the recorded background
        steps), byte for byte.  `pattern_index`: integers in [0, m_all) or None (every pattern in order); `rows`, `cols`:
        (first, step, count) or None (the whole axis).  `into` None: the selection replaces the resident patterns and the
        problem takes its detector shape; another `Context` on this device: that one receives it and this one stays as
        it is (include/kpdi.h, kpdi_select_patterns)."""
        dst = self if into is None else into
        sy, sx = getattr(self, "_detector", (0, 0))  # (nothing set yet: the library refuses the call)
        r0, rs, nr = (0, 1, sy) if rows is None else (int(v) for v in rows)
        c0, cs, nc = (0, 1, sx) if cols is None else (int(v) for v in cols)
        idx = None if pattern_index is None else np.ascontiguousarray(pattern_index, dtype=np.int64).ravel()
        n_out = int(getattr(self, "_exp_shape", (0,))[0]) if idx is None else int(idx.size)
        check(self._f.select_patterns(self._h, dst._h, _ptr(idx), n_out, r0, rs, nr, c0, cs, nc))
        if dst is not self and getattr(dst, "_detector", None) != (nr, nc):  # dst took src's problem with the new shape
            dst._keep_n, dst._compute = self._keep_n, self._compute
        dst._detector = (nr, nc)
        dst._exp_shape, dst._exp_dtype = (n_out, nr, nc), self._exp_dtype

    def set_navigation_mask(self, navigation_mask=None):
        """The navigation mask (True = not matched; None: no mask) of the resident patterns, without a new upload; the
        recorded background steps run first (include/kpdi.h, kpdi_set_navigation_mask)."""
        nm = _mask_bytes(navigation_mask)
        if nm is not None and nm.size != int(self._exp_shape[0]):
            raise KpdiError(f"navigation mask has {nm.size} elements, there are {self._exp_shape[0]} patterns")
        check(self._f.set_navigation_mask(self._h, _ptr(nm)))

    def decomposition_gram(self, centre=CENTRE_NONE):
        """The float64 Gram matrix of the centred resident patterns over their shorter side: (gram (side, side), the
        means that `centre` removed or None, transposed) - `transposed` False: Xc^T Xc over the pixels, True: Xc Xc^T
        over the patterns (include/kpdi.h, kpdi_decomposition_gram).  The resident patterns stay as they are."""
        m, k = int(self._exp_shape[0]), int(np.prod(self._detector))
        side = min(m, k)
        if side > DECOMPOSITION_MAX_SIDE:  # (the library's refusal, before a side x side array is asked for)
            raise KpdiError(f"decomposition of {m} patterns of {k} pixels: the Gram matrix would have {side} rows, above "
                            f"the limit of {DECOMPOSITION_MAX_SIDE} (it is solved on the host); bin the patterns first "
                            "(downsample)")
        gram = np.empty((side, side), dtype=np.float64)
        mean = None if centre == CENTRE_NONE else np.empty(m if centre == CENTRE_SIGNAL else k, dtype=np.float64)
        n, t = C.c_int64(0), C.c_int(0)
        check(self._f.decomposition_gram(self._h, int(centre), _ptr(gram), _ptr(mean), C.byref(n), C.byref(t)))
        return gram, mean, bool(t.value)

    def decomposition_apply(self, basis, centre=CENTRE_NONE, transposed_op=False):
        """Xc basis ((pixels, c) -> (patterns, c)) or, `transposed_op`, Xc^T basis ((patterns, c) -> (pixels, c)) in
        float64, Xc the resident patterns centred as in `decomposition_gram` (include/kpdi.h,
        kpdi_decomposition_apply)."""
        m, k = int(self._exp_shape[0]), int(np.prod(self._detector))
        b = np.ascontiguousarray(basis, dtype=np.float64)
        rows_in, rows_out = (m, k) if transposed_op else (k, m)
        if b.ndim != 2 or b.shape[0] != rows_in:
            raise KpdiError(f"basis of shape {b.shape}: ({rows_in}, c) expected")
        out = np.empty((rows_out, b.shape[1]), dtype=np.float64)
        check(self._f.decomposition_apply(self._h, int(centre), int(bool(transposed_op)), _ptr(b), int(b.shape[1]), _ptr(out)))
        return out

    def decomposition_model(self, loadings, factors, mean=None, mean_kind=CENTRE_NONE, dtype_out=np.float32):
        """Every resident pattern becomes loadings[m] . factors[k] + mean, summed in float64 and rounded once to
        `dtype_out` (float32 / float64), the resident patterns' new dtype; `mean`: None, or the float64 means per pixel
        (`mean_kind` CENTRE_NAVIGATION) or per pattern (CENTRE_SIGNAL) (include/kpdi.h, kpdi_decomposition_model)."""
        dt = np.dtype(dtype_out)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise KpdiError(f"dtype_out {dt}: the decomposition model is written as float32 or float64")
        m, k = int(self._exp_shape[0]), int(np.prod(self._detector))
        lo, fa = np.ascontiguousarray(loadings, dtype=dt), np.ascontiguousarray(factors, dtype=dt)
        if lo.ndim != 2 or fa.ndim != 2 or lo.shape[0] != m or fa.shape[0] != k or lo.shape[1] != fa.shape[1]:
            raise KpdiError(f"loadings {lo.shape} and factors {fa.shape}: ({m}, c) and ({k}, c) expected")
        mu = None
        if mean is not None:
            mu = np.ascontiguousarray(mean, dtype=np.float64).ravel()
            want = {CENTRE_NAVIGATION: k, CENTRE_SIGNAL: m}.get(mean_kind)
            if want is None or mu.size != want:
                raise KpdiError(f"mean of {mu.size} values with mean_kind {mean_kind}")
        check(self._f.decomposition_model(self._h, _ptr(lo), _ptr(fa), int(lo.shape[1]), _ptr(mu), int(mean_kind),
                                          dtype_code(dt)))
        self._exp_dtype = dt

    def kinematical_master_pattern(self, unit_vectors, theta, intensity, half_size, hemisphere):
        """The kinematical master pattern in the stereographic projection from m reflectors (unit normals (m, 3), Bragg
        angles, intensities; float64): (size, size) float64, or (2, size, size) for hemisphere "both", size =
        2 half_size + 1 (include/kpdi.h, kpdi_kinematical_master_pattern).  Independent of the resident patterns."""
        u = np.ascontiguousarray(unit_vectors, dtype=np.float64)
        th = np.ascontiguousarray(theta, dtype=np.float64).ravel()
        inten = np.ascontiguousarray(intensity, dtype=np.float64).ravel()
        if u.ndim != 2 or u.shape[1] != 3 or th.size != u.shape[0] or inten.size != u.shape[0]:
            raise KpdiError(f"unit vectors {u.shape}, {th.size} Bragg angles and {inten.size} intensities: (m, 3), m and "
                            "m expected")
        code = HEMISPHERE_CODES[hemisphere]
        half_size = int(half_size)
        size = 2 * max(half_size, 0) + 1
        if half_size > KINEMATICAL_MAX_HALF_SIZE:  # (the library's refusal, before the output is asked for)
            size = 1
        out = np.empty((2, size, size) if code == 2 else (size, size), dtype=np.float64)
        check(self._f.kinematical_master_pattern(self._h, _ptr(u), _ptr(th), _ptr(inten), u.shape[0], half_size, code,
                                                 _ptr(out)))
        return out

    def sample_fundamental(self, semi_edge_steps, faces):
        """The cubochoric grid of `semi_edge_steps` points per semi-edge, kept where |q_v . a| <= tan(w / 4) q_0 + 1e-9
        for every row (a_x, a_y, a_z, tan(w / 4)) of `faces` ((f, 4) float64, f = 0 keeps every point): (N, 4) float64
        unit quaternions, q_0 >= 0, in lexicographic grid order (include/kpdi.h, kpdi_sample_fundamental_count and
        _fill).  Independent of the resident patterns."""
        fa = np.ascontiguousarray(faces, dtype=np.float64).reshape(-1, 4)
        n, nf = int(semi_edge_steps), int(fa.shape[0])
        count = _i64(0)
        check(self._f.sample_fundamental_count(self._h, n, _ptr(fa) if nf else None, nf, C.byref(count)))
        out = np.empty((count.value, 4), dtype=np.float64)
        check(self._f.sample_fundamental_fill(self._h, n, _ptr(fa) if nf else None, nf, _ptr(out), count.value,
                                              C.byref(count)))
        return out

    @staticmethod
    def _orientation_ops(ops):
        o = np.ascontiguousarray(ops, dtype=np.float64).reshape(-1, 4)
        return o, int(o.shape[0])

    def orientation_pairs(self, q1, q2, shape, stride1, stride2, ops1, ops2, degrees=False):
        """Disorientation angles of a broadcast pair call (include/kpdi.h, kpdi_orientation_pairs): `q1` (rows1, 4) and
        `q2` (rows2, 4) float64; output element (i_0, ...) of `shape` takes the rows sum_d i_d stride1[d] and
        sum_d i_d stride2[d]; `ops1`, `ops2` (n, 4) the groups' operations (equal groups: `ops1` the identity alone).
        Returns float64 of `shape`."""
        a = np.ascontiguousarray(q1, dtype=np.float64).reshape(-1, 4)
        b = np.ascontiguousarray(q2, dtype=np.float64).reshape(-1, 4)
        (o1, n1), (o2, n2) = self._orientation_ops(ops1), self._orientation_ops(ops2)
        shape = tuple(int(v) for v in shape)
        sh, s1, s2 = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (shape, stride1, stride2))
        out = np.empty(shape, dtype=np.float64)
        check(self._f.orientation_pairs(self._h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], len(shape), _ptr(sh), _ptr(s1),
                                        _ptr(s2), _ptr(o1), n1, _ptr(o2), n2, int(bool(degrees)), _ptr(out)))
        return out

    def orientation_outer(self, q1, q2, ops1, ops2, degrees=False, dtype_out=np.float64):
        """The (n, m) disorientation angles of every row of `q1` with every row of `q2` (include/kpdi.h,
        kpdi_orientation_outer), float64 or float32."""
        a = np.ascontiguousarray(q1, dtype=np.float64).reshape(-1, 4)
        b = np.ascontiguousarray(q2, dtype=np.float64).reshape(-1, 4)
        (o1, n1), (o2, n2) = self._orientation_ops(ops1), self._orientation_ops(ops2)
        dt = np.dtype(dtype_out)
        out = np.empty((a.shape[0], b.shape[0]), dtype=dt)
        check(self._f.orientation_outer(self._h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(o1), n1, _ptr(o2), n2,
                                        int(bool(degrees)), dtype_code(dt), _ptr(out)))
        return out

    def orientation_reduce(self, q, ops):
        """((n, 4) float64 equivalents with the largest |a|, a >= 0; (n,) int32 operation indices, -1 for NaN rows) of the
        rows of `q` (include/kpdi.h, kpdi_orientation_reduce)."""
        a = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4)
        o, n = self._orientation_ops(ops)
        out, index = np.empty_like(a), np.empty(a.shape[0], dtype=np.int32)
        check(self._f.orientation_reduce(self._h, _ptr(a), a.shape[0], _ptr(o), n, _ptr(out), _ptr(index)))
        return out, index

    def orientation_kam(self, q, ny, nx, ops, offsets, in_data=None, max_angle=None, degrees=False):
        """The (ny, nx) float64 map of mean disorientation angles to the neighbours at `offsets` ((k, 2) int32 (dy, dx))
        (include/kpdi.h, kpdi_orientation_kam); `max_angle` in radians or None."""
        a = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4)
        o, n = self._orientation_ops(ops)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 2)
        mask = None if in_data is None else np.ascontiguousarray(in_data, dtype=np.uint8).reshape(-1)
        if a.shape[0] != int(ny) * int(nx) or (mask is not None and mask.size != a.shape[0]):
            raise KpdiError(f"{a.shape[0]} rotations for a map of {ny} x {nx} points")
        out = np.empty((int(ny), int(nx)), dtype=np.float64)
        check(self._f.orientation_kam(self._h, _ptr(a), int(ny), int(nx), _ptr(o), n, _ptr(off) if off.shape[0] else None,
                                      int(off.shape[0]), _ptr(mask), -1.0 if max_angle is None else float(max_angle),
                                      int(bool(degrees)), _ptr(out)))
        return out

    def hough_bands(self, n_rho, cos_sin, theta_taps, rho_taps, rim, n_bands, return_sinograms=False):
        """The `n_bands` strongest bands of every resident pattern (include/kpdi.h, kpdi_hough_bands): (m_all, n_bands) of
        `HOUGH_BAND_DTYPE`; with `return_sinograms` also the (m_all, n_theta, n_rho) float32 sinograms.  `cos_sin`
        (2, n_theta) and the two odd-length tap tables are float32."""
        m = int(self._exp_shape[0])
        cs = np.ascontiguousarray(cos_sin, dtype=np.float32)
        wt, wr = (np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in (theta_taps, rho_taps))
        if cs.ndim != 2 or cs.shape[0] != 2 or wt.size % 2 != 1 or wr.size % 2 != 1:
            raise KpdiError(f"cos_sin of shape {cs.shape}, {wt.size} and {wr.size} taps: (2, n_theta) and odd numbers of taps")
        n_theta = cs.shape[1]
        bands = np.zeros((m, int(n_bands)), dtype=HOUGH_BAND_DTYPE)
        sino = np.empty((m, int(n_theta), int(n_rho)), dtype=np.float32) if return_sinograms else None
        check(self._f.hough_bands(self._h, n_theta, int(n_rho), _ptr(cs), _ptr(wt), wt.size // 2, _ptr(wr), wr.size // 2, int(rim),
                                  int(n_bands), _ptr(bands), _ptr(sino)))
        return (bands, sino) if return_sinograms else bands

    def hough_index(self, bands, pcs, shape, sample_to_detector, normals, family, angles, tol):
        """Orientations from bands under one phase (include/kpdi.h, kpdi_hough_index): `bands` (m, n_bands) of
        `HOUGH_BAND_DTYPE`, `pcs` (1 or m, 3).  Returns (quat (m, 4), fit (m,), cm (m,), nmatch (m,) int32)."""
        b = np.ascontiguousarray(bands, dtype=HOUGH_BAND_DTYPE)
        m, nb = b.shape
        pc = np.ascontiguousarray(pcs, dtype=np.float64).reshape(-1, 3)
        s2d = np.ascontiguousarray(sample_to_detector, dtype=np.float64).reshape(3, 3)
        g = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        fam = np.ascontiguousarray(family, dtype=np.int32).reshape(-1)
        ang = np.ascontiguousarray(angles, dtype=np.float64)
        if fam.size != g.shape[0] or ang.shape != (g.shape[0], g.shape[0]):
            raise KpdiError(f"{g.shape[0]} reflectors with {fam.size} families and angles of shape {ang.shape}")
        quat, fit, cm = np.empty((m, 4)), np.empty(m), np.empty(m)
        nmatch = np.empty(m, dtype=np.int32)
        check(self._f.hough_index(self._h, _ptr(b), m, nb, _ptr(pc), pc.shape[0], int(shape[0]), int(shape[1]), _ptr(s2d),
                                  _ptr(g), _ptr(fam), g.shape[0], int(fam.max()) + 1, _ptr(ang), float(tol), _ptr(quat),
                                  _ptr(fit), _ptr(cm), _ptr(nmatch)))
        return quat, fit, cm, nmatch

    def hough_optimize_pc(self, bands, pc0, shape, sample_to_detector, normals, family, angles, tol, xatol=1e-3, fatol=1e-3,
                          maxiter=None, maxfev=None, evals_per_launch=0, lanes=0):
        """One Nelder-Mead search over the projection centre per pattern, on the device (include/kpdi.h,
        kpdi_hough_optimize_pc): `bands` (m, n_bands) of `HOUGH_BAND_DTYPE`, `pc0` (3,), the rest as `hough_index`.
        `maxiter`, `maxfev`: None = unset, as in SciPy.  `evals_per_launch` (0: $KPDI_HOUGH_SEARCH_EVALS, else
        `HOUGH_SEARCH_EVALS`) and `lanes` per workgroup (0: from the plan) bound a kernel's duration and lay the
        searches on the chip; the result does not depend on them.  Returns (pc (m, 3), fun (m,), nfev, nit, status (m,) int32)."""
        b = np.ascontiguousarray(bands, dtype=HOUGH_BAND_DTYPE)
        m, nb = b.shape
        start = np.ascontiguousarray(pc0, dtype=np.float64).reshape(3)
        s2d = np.ascontiguousarray(sample_to_detector, dtype=np.float64).reshape(3, 3)
        g = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
        fam = np.ascontiguousarray(family, dtype=np.int32).reshape(-1)
        ang = np.ascontiguousarray(angles, dtype=np.float64)
        if fam.size != g.shape[0] or ang.shape != (g.shape[0], g.shape[0]):
            raise KpdiError(f"{g.shape[0]} reflectors with {fam.size} families and angles of shape {ang.shape}")
        budget = [0 if v is None else int(min(v, 2**31 - 1)) for v in (maxiter, maxfev)]
        if min(budget) < 0 or any(v is not None and v < 1 for v in (maxiter, maxfev)):
            raise KpdiError(f"maxiter {maxiter} and maxfev {maxfev}: None or at least 1")
        pc, fun = np.empty((m, 3)), np.empty(m)
        nfev, nit, status = (np.empty(m, dtype=np.int32) for _ in range(3))
        check(self._f.hough_optimize_pc(self._h, _ptr(b), m, nb, _ptr(start), int(shape[0]), int(shape[1]), _ptr(s2d), _ptr(g),
                                        _ptr(fam), g.shape[0], int(fam.max()) + 1, _ptr(ang), float(tol), float(np.degrees(tol)),
                                        float(xatol), float(fatol), budget[0], budget[1], int(evals_per_launch), int(lanes),
                                        _ptr(pc), _ptr(fun), _ptr(nfev), _ptr(nit), _ptr(status)))
        return pc, fun, nfev, nit, status

    @staticmethod
    def _geometrical_inputs(rotations, u_s, pcs, *bases):
        rot = np.ascontiguousarray(rotations, dtype=np.float64)
        pc = np.ascontiguousarray(pcs, dtype=np.float64)
        mats = [np.ascontiguousarray(a, dtype=np.float64) for a in (u_s,) + bases]
        if rot.ndim != 2 or rot.shape[1] != 4 or pc.ndim != 2 or pc.shape[1] != GEOMETRICAL_PC_DOUBLES:
            raise KpdiError(f"rotations {rot.shape} and projection centre table {pc.shape}: (n, 4) and (1 or n, "
                            f"{GEOMETRICAL_PC_DOUBLES}) expected")
        if any(a.shape != (3, 3) for a in mats):
            raise KpdiError(f"matrices of shapes {[a.shape for a in mats]}: (3, 3) expected")
        return rot, pc, mats

    def geometrical_visibility(self, vectors, kind, rotations, u_s, basis, pcs):
        """Which of m features are in some pattern of a map (include/kpdi.h, kpdi_geometrical_visibility): `vectors`
        (m, 3) hkl with `basis` rows a*, b*, c* (`kind` GEOMETRICAL_LINES) or uvw with rows a, b, c
        (GEOMETRICAL_ZONE_AXES); `rotations` (n, 4); `u_s` the sample-to-detector matrix transposed; `pcs` (1 or n, 8).
        Returns m uint8 flags: GEOMETRICAL_UPPER | GEOMETRICAL_INSIDE."""
        v = np.ascontiguousarray(vectors, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 3:
            raise KpdiError(f"vectors {v.shape}: (m, 3) expected")
        rot, pc, (us, b) = self._geometrical_inputs(rotations, u_s, pcs, basis)
        flags = np.zeros(v.shape[0], dtype=np.uint8)
        check(self._f.geometrical_visibility(self._h, _ptr(v), v.shape[0], int(kind), _ptr(rot), rot.shape[0], _ptr(us),
                                             _ptr(b), _ptr(pc), pc.shape[0], _ptr(flags)))
        return flags

    def geometrical_coordinates(self, hkl, uvw, rotations, u_s, a_star, a_direct, pcs, r_gnomonic):
        """Lines and zone axes of every map point on the detector (include/kpdi.h, kpdi_geometrical_coordinates): a dict
        of `line_in_pattern` (n, m) bool, `line_gnomonic` and `line_pixel` (n, m, 4), `zone_in_pattern` (n, z) bool,
        `zone_gnomonic` and `zone_pixel` (n, z, 2); float64, NaN where the reference has NaN."""
        h = np.ascontiguousarray(hkl, dtype=np.float64)
        w = np.ascontiguousarray(uvw, dtype=np.float64).reshape(-1, 3)
        if h.ndim != 2 or h.shape[1] != 3:
            raise KpdiError(f"hkl {h.shape}: (m, 3) expected")
        rot, pc, (us, a_s, a_d) = self._geometrical_inputs(rotations, u_s, pcs, a_star, a_direct)
        n, m, z = rot.shape[0], h.shape[0], w.shape[0]
        out = {"line_in_pattern": np.zeros((n, m), dtype=np.uint8), "line_gnomonic": np.empty((n, m, 4)),
               "line_pixel": np.empty((n, m, 4)), "zone_in_pattern": np.zeros((n, z), dtype=np.uint8),
               "zone_gnomonic": np.empty((n, z, 2)), "zone_pixel": np.empty((n, z, 2))}
        check(self._f.geometrical_coordinates(self._h, _ptr(h), m, _ptr(w) if z else None, z, _ptr(rot), n, _ptr(us),
                                              _ptr(a_s), _ptr(a_d), _ptr(pc), pc.shape[0], float(r_gnomonic),
                                              _ptr(out["line_in_pattern"]), _ptr(out["line_gnomonic"]),
                                              _ptr(out["line_pixel"]), *((_ptr(out[k]) if z else None) for k in
                                                                         ("zone_in_pattern", "zone_gnomonic", "zone_pixel"))))
        out["line_in_pattern"] = out["line_in_pattern"].view(np.bool_)
        out["zone_in_pattern"] = out["zone_in_pattern"].view(np.bool_)
        return out

    def normalize_intensity(self, num_std=1, divide_by_square_root=False, dtype_out=None):
        """(p - mean) / (num_std * std [* sqrt(size)]) of every resident pattern into `dtype_out` (None: the patterns'
        dtype); the resident patterns take the new dtype (include/kpdi.h, kpdi_normalize_intensity)."""
        dt = self._exp_dtype if dtype_out is None else np.dtype(dtype_out)
        check(self._f.normalize_intensity(self._h, float(num_std), int(bool(divide_by_square_root)), dtype_code(dt)))
        self._exp_dtype = dt

    def intensity_range(self):
        """(min, max) over every resident pattern, NaN if any value is NaN: float64 (2,)."""
        out = np.empty(2, dtype=np.float64)
        check(self._f.intensity_range(self._h, _ptr(out)))
        return out

    def adaptive_histogram_equalization(self, ky, kx, clip_count, nbins):
        """Equalize every resident pattern in place (after the recorded background steps) with a `ky` x `kx` kernel,
        the integer clip limit `clip_count` (>= ky * kx: none) and `nbins` bins; the dtype stays (include/kpdi.h,
        kpdi_adaptive_histogram_equalization)."""
        check(self._f.adaptive_histogram_equalization(self._h, int(ky), int(kx), int(clip_count), int(nbins)))

    def average_neighbour_patterns(self, ny, nx, window, window_sums, row0=0, row1=None):
        """Average every resident pattern of the rows [row0, row1) of the ny x nx map with its neighbours under the
        2-D `window` (float64 coefficients, origin at shape // 2) and rescale it to its dtype's range; `window_sums`:
        (ny, nx) integers, the truncated window sum of every resident point taken from the WHOLE map.  The averaged
        patterns replace the resident ones (include/kpdi.h, kpdi_average_neighbour_patterns)."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        ws = np.ascontiguousarray(window_sums, dtype=np.int64)
        if w.ndim != 2:
            raise KpdiError(f"window of shape {w.shape}")
        if ws.size != int(ny) * int(nx):
            raise KpdiError(f"{ws.size} window sums for a map of {ny} x {nx} points")
        check(self._f.average_neighbour_patterns(self._h, int(ny), int(nx), _ptr(w), int(w.shape[0]), int(w.shape[1]),
                                                 _ptr(ws), int(row0), int(ny if row1 is None else row1)))

    def neighbour_dot_products(self, ny, nx, footprint, zero_mean=True, normalize=True, dtype_out=np.float32, row0=0,
                               row1=None, matrices=True, average=True):
        """Dot products of every resident pattern of the rows [row0, row1) of the ny x nx map with its neighbours under
        the 2-D boolean `footprint`: (matrices (rows, nx, wy, wx) or None, average map (rows, nx) or None) of
        `dtype_out` (float32 / float64), from one launch (include/kpdi.h, kpdi_neighbour_dot_products)."""
        fp = np.ascontiguousarray(np.asarray(footprint) != 0, dtype=np.uint8)
        dt = np.dtype(dtype_out)
        if fp.ndim != 2:
            raise KpdiError(f"footprint of shape {fp.shape}")
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise KpdiError(f"dtype_out {dt}: the dot products are float32 or float64")
        row1 = int(ny if row1 is None else row1)
        rows = max(row1 - int(row0), 0)
        mat = np.empty((rows, int(nx)) + fp.shape, dtype=dt) if matrices else None
        adp = np.empty((rows, int(nx)), dtype=dt) if average else None
        check(self._f.neighbour_dot_products(self._h, int(ny), int(nx), _ptr(fp), int(fp.shape[0]), int(fp.shape[1]),
                                             int(bool(zero_mean)), int(bool(normalize)), int(dt == np.float64),
                                             int(row0), row1, _ptr(mat), _ptr(adp)))
        return mat, adp

    # -- sweep
    def set_dictionary_size(self, n_total):
        """How many dictionary patterns the coming sweep pushes in total.  One context sweeps them all whatever the
        number; a `Group` plans its chunk assignment with it."""

    def push_dictionary_chunk(self, patterns, global_start):
        p = np.ascontiguousarray(patterns)
        # returns when the upload has consumed `p`; the sweep of the chunk runs on
        check(self._f.push_dictionary_chunk(self._h, _ptr(p), dtype_code(p.dtype), p.shape[0],
                                                int(global_start)))

    def push_dictionary_chunk_dev(self, d_ptr, dtype, n_chunk, global_start):
        check(self._f.push_dictionary_chunk_dev(self._h, C.c_void_p(d_ptr), dtype_code(dtype),
                                                    int(n_chunk), int(global_start)))

    # -- resident dictionary: prepared once, swept against several experimental sets
    def hold_dictionary_chunk(self, patterns, global_start):
        p = np.ascontiguousarray(patterns)
        check(self._f.hold_dictionary_chunk(self._h, _ptr(p), dtype_code(p.dtype), p.shape[0],
                                                int(global_start)))

    def hold_dictionary_chunk_dev(self, d_ptr, dtype, n_chunk, global_start):
        check(self._f.hold_dictionary_chunk_dev(self._h, C.c_void_p(d_ptr), dtype_code(dtype),
                                                    int(n_chunk), int(global_start)))

    def hold_rotations_chunk(self, rotations, global_start, rescale=False, out_min=-1.0, out_max=1.0):
        rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        check(self._f.hold_rotations_chunk(self._h, _ptr(rot), rot.shape[0], int(global_start),
                                               int(bool(rescale)), float(out_min), float(out_max)))

    def sweep_held(self):
        check(self._f.sweep_held(self._h))

    def release_held(self):
        check(self._f.release_held(self._h))

    def held_size(self):
        """(patterns held, bytes of device memory they occupy)."""
        n, b = C.c_int64(0), C.c_int64(0)
        check(self._f.held_size(self._h, C.byref(n), C.byref(b)))
        return n.value, b.value

    # -- dictionary generation on the device
    def set_master_pattern(self, upper, lower=None):
        """upper / lower: (npy, npx) arrays of one dtype (uint8, uint16, float32, float64)."""
        up = np.ascontiguousarray(upper)
        lo = None if lower is None else np.ascontiguousarray(lower, dtype=up.dtype)
        if up.ndim != 2 or (lo is not None and lo.shape != up.shape):
            raise KpdiError("master pattern hemispheres must be 2D arrays of equal shape")
        self._projection_key = None  # whoever cached "my master pattern is loaded" must load it again
        check(self._f.set_master_pattern(self._h, _ptr(up), _ptr(lo), dtype_code(up.dtype),
                                             up.shape[1], up.shape[0]))

    def set_detector(self, gnomonic_bounds, pcz, nrows, ncols, om_detector_to_sample):
        gb = np.ascontiguousarray(gnomonic_bounds, dtype=np.float64).ravel()
        om = np.ascontiguousarray(om_detector_to_sample, dtype=np.float64).ravel()
        if gb.size != 4 or om.size != 9:
            raise KpdiError("gnomonic_bounds must have 4 and om_detector_to_sample 9 elements")
        self._projection_key = None
        check(self._f.set_detector(self._h, _ptr(gb), float(pcz), int(nrows), int(ncols), _ptr(om)))
        self._dc_npix = int(nrows) * int(ncols)

    def set_direction_cosines(self, direction_cosines):
        dc = np.ascontiguousarray(direction_cosines, dtype=np.float64).reshape(-1, 3)
        self._projection_key = None
        check(self._f.set_direction_cosines(self._h, _ptr(dc), dc.shape[0]))
        self._dc_npix = dc.shape[0]

    def get_direction_cosines(self):
        out = np.empty((self._dc_npix, 3), dtype=np.float64)
        check(self._f.get_direction_cosines(self._h, _ptr(out)))
        return out

    def project_patterns(self, rotations, rescale=False, out_min=-1.0, out_max=1.0, dtype_out=np.float32):
        rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        out = np.empty((rot.shape[0], self._dc_npix), dtype=dtype_out)
        check(self._f.project_patterns(self._h, _ptr(rot), rot.shape[0], int(bool(rescale)),
                                           float(out_min), float(out_max), dtype_code(out.dtype), _ptr(out)))
        return out

    def project_patterns_varying_pc(self, rotations, pcs, shape, om_detector_to_sample, rescale=False, out_min=-1.0,
                                    out_max=1.0, dtype_out=np.float32):
        rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        pc = np.ascontiguousarray(pcs, dtype=np.float64).reshape(-1, 3)
        if pc.shape[0] != rot.shape[0]:
            raise KpdiError(f"{rot.shape[0]} rotations but {pc.shape[0]} projection centres")
        om = np.ascontiguousarray(om_detector_to_sample, dtype=np.float64).ravel()
        out = np.empty((rot.shape[0], shape[0] * shape[1]), dtype=dtype_out)
        check(self._f.project_patterns_varying_pc(self._h, _ptr(rot), _ptr(pc), rot.shape[0], int(shape[0]),
                                                      int(shape[1]), _ptr(om), int(bool(rescale)), float(out_min),
                                                      float(out_max), dtype_code(out.dtype), _ptr(out)))
        return out

    def push_rotations_chunk(self, rotations, global_start, rescale=False, out_min=-1.0, out_max=1.0):
        rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        check(self._f.push_rotations_chunk(self._h, _ptr(rot), rot.shape[0], int(global_start),
                                               int(bool(rescale)), float(out_min), float(out_max)))

    def push_rotations_chunk_varying_pc(self, rotations, pcs, global_start, om_detector_to_sample, rescale=False,
                                        out_min=-1.0, out_max=1.0):
        """A dictionary chunk simulated on the device with ONE projection centre per pattern, then swept."""
        rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        pc = np.ascontiguousarray(pcs, dtype=np.float64).reshape(-1, 3)
        if pc.shape[0] != rot.shape[0]:
            raise KpdiError(f"{rot.shape[0]} rotations but {pc.shape[0]} projection centres")
        om = np.ascontiguousarray(om_detector_to_sample, dtype=np.float64).ravel()
        if om.size != 9:
            raise KpdiError("om_detector_to_sample must have 9 elements")
        check(load().kpdi_push_rotations_chunk_varying_pc(self._h, _ptr(rot), _ptr(pc), rot.shape[0], int(global_start), _ptr(om),
                                                          int(bool(rescale)), float(out_min), float(out_max)))

    # -- refinement
    def refine_set_patterns(self, patterns, signal_mask=None, rescale=False, om_detector_to_sample=None):
        """patterns: (n, nrows, ncols); signal_mask: True = pixel not used."""
        p = np.ascontiguousarray(patterns)
        if p.ndim != 3:
            raise KpdiError("patterns must have shape (n, nrows, ncols)")
        sm = _mask_bytes(signal_mask)
        om = np.ascontiguousarray(om_detector_to_sample, dtype=np.float64).ravel()
        if om.size != 9:
            raise KpdiError("om_detector_to_sample must have 9 elements")
        check(self._f.refine_set_patterns(self._h, _ptr(p), dtype_code(p.dtype), p.shape[0], p.shape[1],
                                              p.shape[2], _ptr(sm), int(bool(rescale)), _ptr(om)))
        self._ref_n = p.shape[0]
        self._ref_k = p.shape[1] * p.shape[2] if sm is None else int(np.count_nonzero(sm == 0))

    def refine_get_prepared(self):
        pat = np.empty((self._ref_n, self._ref_k), dtype=np.float32)
        sqn = np.empty(self._ref_n, dtype=np.float64)
        check(self._f.refine_get_prepared(self._h, _ptr(pat), _ptr(sqn)))
        return pat, sqn

    def refine_objective(self, mode, pattern_index, x, fixed=None):
        idx = np.ascontiguousarray(pattern_index, dtype=np.int32).ravel()
        nvar, nfixed = REFINE_SIZES[mode]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(idx.size, nvar)
        f = None if nfixed == 0 else np.ascontiguousarray(fixed, dtype=np.float64).reshape(idx.size, nfixed)
        out = np.empty(idx.size, dtype=np.float64)
        check(self._f.refine_objective(self._h, int(mode), idx.size, _ptr(idx), _ptr(x), _ptr(f), _ptr(out)))
        return out

    @staticmethod
    def _solve_arrays(mode, x0, fixed, lower, upper):
        """The arrays of a batch of solves, shaped for the library: nvar, x0 (n_patterns, n_starts, nvar), fixed,
        lower, upper (or None) and the empty result rows."""
        nvar, nfixed = REFINE_SIZES[mode]
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.ndim != 3 or x0.shape[2] != nvar:
            raise KpdiError(f"x0 must have shape (n_patterns, n_starts, {nvar})")
        n, starts = x0.shape[:2]
        f = None if nfixed == 0 else np.ascontiguousarray(fixed, dtype=np.float64).reshape(n, starts, nfixed)
        lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(x0.shape)
        hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(x0.shape)
        return nvar, x0, f, lo, hi, np.empty((n, starts, REFINE_RESULT_STRIDE), dtype=np.float64)

    @staticmethod
    def _trace_buffer(nvar, trace_job, trace_capacity):
        """The (trace_capacity, nvar + 1) rows a traced solve fills, or None without a `trace_job`."""
        if trace_job is None:
            return None
        if int(trace_capacity) < 1:
            raise KpdiError("a trace needs trace_capacity >= 1")
        return np.zeros((int(trace_capacity), nvar + 1), dtype=np.float64)

    @staticmethod
    def _with_trace(res, trace, trace_job):
        """`res`, or with a trace (res, the rows of it that were stored, how many evaluations `trace_job` made: its nfev)."""
        if trace is None:
            return res
        total = int(res.reshape(-1, res.shape[2])[int(trace_job), 1])
        return res, trace[:min(total, trace.shape[0])], total

    def _optimiser_selftest(self, entry, n_head, kind, x0, lower, upper, xtol, ftol, maxiter, maxfev):
        """One optimiser alone on an analytic objective: `n_head` result fields, then x."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).ravel()
        lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).ravel()
        hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).ravel()
        res = np.empty(n_head + x0.size, dtype=np.float64)
        check(entry(self._h, int(kind), x0.size, _ptr(x0), _ptr(lo), _ptr(hi), float(xtol), float(ftol),
                    int(maxiter or 0), int(maxfev or 0), _ptr(res)))
        return res

    def refine_solve(self, mode, x0, fixed=None, lower=None, upper=None, xatol=1e-4, fatol=1e-4, maxiter=0,
                     maxfev=0):
        """x0: (n_patterns, n_starts, nvar).  Returns (n_patterns, n_starts, 3 + nvar):
        fun, nfev, nit, x."""
        nvar, x0, f, lo, hi, res = self._solve_arrays(mode, x0, fixed, lower, upper)
        check(self._f.refine_solve(self._h, int(mode), x0.shape[0], x0.shape[1], _ptr(x0), _ptr(f), _ptr(lo), _ptr(hi),
                                   float(xatol), float(fatol), int(maxiter or 0), int(maxfev or 0), _ptr(res)))
        return res[:, :, :3 + nvar]

    def nelder_mead_selftest(self, kind, x0, lower=None, upper=None, xatol=1e-4, fatol=1e-4, maxiter=0, maxfev=0):
        return self._optimiser_selftest(self._f.nelder_mead_selftest, 3, kind, x0, lower, upper, xatol, fatol, maxiter,
                                        maxfev)

    def refine_solve_powell(self, mode, x0, fixed=None, lower=None, upper=None, xtol=1e-4, ftol=1e-4, maxiter=0,
                            maxfev=0, trace_job=None, trace_capacity=0):
        """`scipy.optimize.minimize(method="Powell")` from every start on the device (kpdi_refine_solve_powell).
        x0: (n_patterns, n_starts, nvar); bounds: none or finite.  Returns the (n_patterns, n_starts, 3 + nvar) rows
        fun, nfev, nit, x.  With `trace_job` (= pattern * n_starts + start) also the (n_stored, nvar + 1) rows (x, f)
        of that job's evaluations, the first `trace_capacity` of them, and how many there were in all."""
        nvar, x0, f, lo, hi, res = self._solve_arrays(mode, x0, fixed, lower, upper)
        trace = self._trace_buffer(nvar, trace_job, trace_capacity)
        check(self._f.refine_solve_powell(self._h, int(mode), x0.shape[0], x0.shape[1], _ptr(x0), _ptr(f), _ptr(lo),
                                          _ptr(hi), float(xtol), float(ftol), int(maxiter or 0), int(maxfev or 0), _ptr(res),
                                          int(trace_job or 0), _ptr(trace), 0 if trace is None else trace.shape[0]))
        return self._with_trace(res[:, :, :3 + nvar], trace, trace_job)

    def powell_selftest(self, kind, x0, lower=None, upper=None, xtol=1e-4, ftol=1e-4, maxiter=0, maxfev=0):
        """csrc/powell.h alone on an analytic objective (kpdi_powell_selftest): fun, nfev, nit, status, x."""
        return self._optimiser_selftest(self._f.powell_selftest, 4, kind, x0, lower, upper, xtol, ftol, maxiter, maxfev)

    def refine_solve_nlopt(self, mode, x0, fixed=None, lower=None, upper=None, xstep=None, ftol_rel=1e-4, maxeval=0):
        """The LN_NELDERMEAD search of csrc/nlopt_simplex.h from every start on the device (kpdi_refine_solve_nlopt).
        x0: (n_patterns, n_starts, nvar); bounds: none or both (infinite allowed); xstep: None (the default step) or
        nvar initial steps.  Returns the (n_patterns, n_starts, 3 + nvar) rows fun, nfev, status, x."""
        nvar, x0, f, lo, hi, res = self._solve_arrays(mode, x0, fixed, lower, upper)
        step = None
        if xstep is not None:
            step = np.ascontiguousarray(xstep, dtype=np.float64).ravel()
            if step.size != nvar:
                raise KpdiError(f"xstep must have {nvar} values")
        check(self._f.refine_solve_nlopt(self._h, int(mode), x0.shape[0], x0.shape[1], _ptr(x0), _ptr(f), _ptr(lo),
                                         _ptr(hi), _ptr(step), float(ftol_rel), int(maxeval or 0), _ptr(res)))
        return res[:, :, :3 + nvar]

    def nlopt_simplex_selftest(self, kind, x0, lower=None, upper=None, xstep=None, ftol_rel=0.0, maxeval=0):
        """csrc/nlopt_simplex.h alone on an analytic objective (kpdi_nlopt_simplex_selftest): fun, nfev, status, x."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).ravel()
        lo, hi, step = (None if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel()
                        for a in (lower, upper, xstep))
        if any(a is not None and a.size != x0.size for a in (lo, hi, step)):
            raise KpdiError("lower, upper and xstep must have one value per variable")
        res = np.empty(3 + x0.size, dtype=np.float64)
        check(self._f.nlopt_simplex_selftest(self._h, int(kind), x0.size, _ptr(x0), _ptr(lo), _ptr(hi), _ptr(step),
                                             float(ftol_rel), int(maxeval or 0), _ptr(res)))
        return res

    @staticmethod
    def _de_mutation(mutation):
        """(lo, hi) as the library takes `mutation`: hi = NaN for one number, else the pair as given."""
        if np.ndim(mutation) == 0:
            return float(mutation), float("nan")
        lo, hi = mutation
        return float(lo), float(hi)

    def refine_solve_de(self, mode, fixed, lower, upper, members, maxiter=1000, tol=0.01, atol=0.0, mutation=(0.5, 1.0),
                        recombination=0.7, init=0, updating=0, seeds=0, trace_job=None, trace_capacity=0):
        """`scipy.optimize.differential_evolution(strategy="best1bin", polish=False)` for every start on the device
        (kpdi_refine_solve_de), job j from `numpy.random.RandomState(seeds[j])`.  lower, upper: (n_patterns, n_starts,
        nvar), finite; members: the population; mutation: a number or the ordered dither pair; init: 0 latinhypercube,
        1 random; updating: 0 immediate, 1 deferred; seeds: one integer for every job or one per job.  Returns the
        (n_patterns, n_starts, 3 + nvar) rows fun, nfev, nit, x, and with `trace_job` the trace as `refine_solve_powell`."""
        if lower is None or upper is None:
            raise KpdiError("differential evolution searches within bounds: give lower and upper")
        nvar, lo, f, _, hi, res = self._solve_arrays(mode, lower, fixed, None, upper)
        n_jobs = lo.shape[0] * lo.shape[1]
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32).ravel(), (n_jobs,)))
        m_lo, m_hi = self._de_mutation(mutation)
        trace = self._trace_buffer(nvar, trace_job, trace_capacity)
        check(self._f.refine_solve_de(self._h, int(mode), lo.shape[0], lo.shape[1], _ptr(f), _ptr(lo), _ptr(hi), int(members),
                                      int(maxiter), float(tol), float(atol), m_lo, m_hi, float(recombination), int(init),
                                      int(updating), _ptr(seeds), _ptr(res), int(trace_job or 0), _ptr(trace),
                                      0 if trace is None else trace.shape[0]))
        return self._with_trace(res[:, :, :3 + nvar], trace, trace_job)

    def de_selftest(self, kind, lower, upper, members, maxiter=1000, tol=0.01, atol=0.0, mutation=(0.5, 1.0),
                    recombination=0.7, init=0, updating=0, seed=0):
        """csrc/differential_evolution.h alone on an analytic objective (kpdi_de_selftest): fun, nfev, nit, success, x."""
        lo = np.ascontiguousarray(lower, dtype=np.float64).ravel()
        hi = np.ascontiguousarray(upper, dtype=np.float64).ravel()
        if lo.size != hi.size:
            raise KpdiError("lower and upper must have one value per variable")
        m_lo, m_hi = self._de_mutation(mutation)
        res = np.empty(4 + lo.size, dtype=np.float64)
        check(self._f.de_selftest(self._h, int(kind), lo.size, _ptr(lo), _ptr(hi), int(members), int(maxiter), float(tol),
                                  float(atol), m_lo, m_hi, float(recombination), int(init), int(updating), int(seed),
                                  _ptr(res)))
        return res

    def refine_solve_basinhopping(self, mode, x0, fixed=None, niter=100, T=1.0, stepsize=0.5, interval=50,
                                  niter_success=None, target_accept_rate=0.5, stepwise_factor=0.9, xatol=1e-4, fatol=1e-4,
                                  maxiter=0, maxfev=0, seeds=0, trace_job=None, trace_capacity=0):
        """`scipy.optimize.basinhopping` around `minimize(method="Nelder-Mead")` from every start on the device
        (kpdi_refine_solve_basinhopping), job j from `numpy.random.RandomState(seeds[j])`, unbounded.  x0: (n_patterns,
        n_starts, nvar); niter_success None: niter + 2; xatol, fatol, maxiter, maxfev: the options of every quench
        (None or 0: SciPy's budget rule); seeds: one integer for every job or one per job.  Returns the (n_patterns,
        n_starts, 3 + nvar) rows fun, nfev, nit, x of the lowest result, and with `trace_job` the trace as
        `refine_solve_powell`."""
        nvar, x0, f, _, _, res = self._solve_arrays(mode, x0, fixed, None, None)
        n_jobs = x0.shape[0] * x0.shape[1]
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32).ravel(), (n_jobs,)))
        trace = self._trace_buffer(nvar, trace_job, trace_capacity)
        check(self._f.refine_solve_basinhopping(self._h, int(mode), x0.shape[0], x0.shape[1], _ptr(x0), _ptr(f), int(niter),
                                                float(T), float(stepsize), int(interval),
                                                -1 if niter_success is None else int(niter_success),
                                                float(target_accept_rate), float(stepwise_factor), float(xatol),
                                                float(fatol), int(maxiter or 0), int(maxfev or 0), _ptr(seeds), _ptr(res),
                                                int(trace_job or 0), _ptr(trace), 0 if trace is None else trace.shape[0]))
        return self._with_trace(res[:, :, :3 + nvar], trace, trace_job)

    def basinhopping_selftest(self, kind, x0, niter=100, T=1.0, stepsize=0.5, interval=50, niter_success=None,
                              target_accept_rate=0.5, stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, maxiter=0, maxfev=0,
                              seed=0):
        """csrc/basinhopping.h alone on an analytic objective (kpdi_basinhopping_selftest): fun, nfev, nit, success,
        minimization_failures, x."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).ravel()
        res = np.empty(5 + x0.size, dtype=np.float64)
        check(self._f.basinhopping_selftest(self._h, int(kind), x0.size, _ptr(x0), int(niter), float(T), float(stepsize),
                                            int(interval), -1 if niter_success is None else int(niter_success),
                                            float(target_accept_rate), float(stepwise_factor), float(xatol), float(fatol),
                                            int(maxiter or 0), int(maxfev or 0), int(seed), _ptr(res)))
        return res

    def mt19937_selftest(self, seed, program):
        """The random stream of csrc/differential_evolution.h alone (kpdi_mt19937_selftest).  program: rows (op, a, b) -
        0: uniform(), 1: uniform(a, b), 2: randint(0, a), 3: shuffle of a persistent arange(a), 4: permutation(range(a)).
        Returns the raw 64 bits of every value drawn (uint64)."""
        prog = np.ascontiguousarray(program, dtype=np.float64).reshape(-1, 3)
        words = int(sum(int(a) if op >= 3 else 1 for op, a, _ in prog))
        out = np.zeros(max(words, 1), dtype=np.uint64)
        check(self._f.mt19937_selftest(self._h, int(seed), _ptr(prog), prog.shape[0], _ptr(out), words))
        return out[:words]

    def merge_selftest(self, sources, m, k, out_scores, out_idx, out_offset=0, segments=None, seg_sources=0, force=-1):
        """merge.hip alone (kpdi_merge_selftest).  sources: up to three dicts of scores (float32), idx (int32), cnt
        (int32 (m, lists) or None), lists, len, row_stride, list_stride; out_scores / out_idx: (m, out_stride), prefilled.
        segments: (row0, delta).  Returns (scores, idx, launch error, kernel that ran)."""
        n = len(sources)
        keep = []

        def table(key, dtype):
            ptrs = (C.c_void_p * 3)()
            for j, src in enumerate(sources):
                if src.get(key) is not None:
                    a = np.ascontiguousarray(src[key], dtype=dtype)
                    keep.append(a)
                    ptrs[j] = a.ctypes.data
            return ptrs

        ps, pi, pc = table("scores", np.float32), table("idx", np.int32), table("cnt", np.int32)
        for j, src in enumerate(sources):
            if src.get("cnt") is not None and np.asarray(src["cnt"]).size != m * src["lists"]:
                raise KpdiError(f"source {j}: counts must have shape (m, lists)")
            if np.asarray(src["scores"]).size != np.asarray(src["idx"]).size:
                raise KpdiError(f"source {j}: scores and idx differ in size")
        ints = {key: np.array([src[key] for src in sources], dtype=np.int32)
                for key in ("lists", "len", "row_stride", "list_stride")}
        elems = np.array([np.asarray(src["scores"]).size for src in sources], dtype=np.int64)
        out_s = np.array(out_scores, dtype=np.float32, order="C")
        out_i = np.array(out_idx, dtype=np.int32, order="C")
        if out_s.shape != out_i.shape or out_s.ndim != 2 or out_s.shape[0] != m:
            raise KpdiError("out_scores / out_idx must have shape (m, out_stride)")
        row0 = delta = None
        if segments is not None:
            row0 = np.ascontiguousarray(segments[0], dtype=np.int32)
            delta = np.ascontiguousarray(segments[1], dtype=np.int32)
        err, ran = C.c_int32(0), C.c_int32(-1)
        check(self._f.merge_selftest(self._h, n, C.addressof(ps), C.addressof(pi), C.addressof(pc), _ptr(elems),
                                     _ptr(ints["lists"]), _ptr(ints["len"]), _ptr(ints["row_stride"]),
                                     _ptr(ints["list_stride"]), int(m), int(k), out_s.shape[1], int(out_offset),
                                     0 if row0 is None else row0.size, _ptr(row0), _ptr(delta), int(seg_sources),
                                     _ptr(out_s), _ptr(out_i), int(force), C.addressof(err), C.addressof(ran)))
        return out_s, out_i, err.value, ran.value

    def merge64_selftest(self, k, cand_s64, cand_i, lists, length, row_stride, list_stride, out_s, out_i, run=None,
                         in_place=False, cert=None):
        """rescore.hip's merge64_kernel alone (kpdi_merge64_selftest).  run: (scores, idx) (m, k) or None; cert: dict of
        cand_s32 (m, s32_stride), s32_col, max_diff, eps_floor, enumerated_all, or None.  Returns (scores, idx,
        uncertified or None, launch error)."""
        out_s = np.array(out_s, dtype=np.float64, order="C")
        out_i = np.array(out_i, dtype=np.int32, order="C")
        m = out_s.shape[0]
        cs = np.ascontiguousarray(cand_s64, dtype=np.float64)
        ci = np.ascontiguousarray(cand_i, dtype=np.int32)
        rs = ri = s32 = None
        if run is not None:
            rs = np.ascontiguousarray(run[0], dtype=np.float64)
            ri = np.ascontiguousarray(run[1], dtype=np.int32)
            if rs.shape != (m, k) or ri.shape != (m, k):
                raise KpdiError("the running list must have shape (m, k)")
        if out_s.shape != (m, k) or out_i.shape != (m, k) or cs.size != ci.size:
            raise KpdiError("out must have shape (m, k); candidate scores and indices the same size")
        unc, err = C.c_int32(0), C.c_int32(0)
        stride = col = 0
        if cert is not None:
            s32 = np.ascontiguousarray(cert["cand_s32"], dtype=np.float32)
            if s32.ndim != 2 or s32.shape[0] != m:
                raise KpdiError("cand_s32 must have shape (m, s32_stride)")
            stride, col = s32.shape[1], int(cert["s32_col"])
        check(self._f.merge64_selftest(self._h, m, int(k), _ptr(rs), _ptr(ri), int(bool(in_place)), _ptr(cs), _ptr(ci),
                                       cs.size, int(lists), int(length), int(row_stride), int(list_stride), _ptr(s32),
                                       stride, col, int(bool(cert and cert.get("enumerated_all"))),
                                       float(cert["max_diff"]) if cert else 0.0, float(cert["eps_floor"]) if cert else 0.0,
                                       _ptr(out_s), _ptr(out_i), C.addressof(unc) if cert is not None else None,
                                       C.addressof(err)))
        return out_s, out_i, (unc.value if cert is not None else None), err.value

    def rescore_selftest(self, exp, dic, metric, cand_s, cand_i, cand_s64, cand_offset=0, n_cand=None, global_start=0,
                         row_map=None, pix_map=None, k=None, max_diff=0.0, exp_dtype=None, dict_dtype=None):
        """rescore.hip's rescore_kernel alone (kpdi_rescore_selftest).  exp: (m_all, npix), dic: (n_chunk, npix), any of
        the nine dtypes (exp_dtype / dict_dtype: a code to pass instead of the array's own); cand_s / cand_i / cand_s64:
        (m, cand_stride), cand_s64 prefilled; k: kept pixels (default: all of pix_map, or npix).  Maps and extents go to
        the library as given: it refuses what would read outside a buffer (and then cand_s64 is as it was).  Returns (cand_s64 after the launch,
        max_diff after the launch as float32, launch error)."""
        exp = np.ascontiguousarray(exp)
        dic = np.ascontiguousarray(dic)
        if exp.ndim != 2 or dic.ndim != 2 or exp.shape[1] != dic.shape[1]:
            raise KpdiError("exp and dic must have shape (rows, npix) with the same npix")
        cs = np.ascontiguousarray(cand_s, dtype=np.float32)
        ci = np.ascontiguousarray(cand_i, dtype=np.int32)
        out = np.require(cand_s64, np.float64, ["C", "W"])  # a writable C-ordered float64 array is filled in place
        if cs.ndim != 2 or ci.shape != cs.shape or out.shape != cs.shape:
            raise KpdiError("cand_s, cand_i and cand_s64 must share the shape (m, cand_stride)")
        m, stride = cs.shape
        rows = None if row_map is None else np.ascontiguousarray(row_map, dtype=np.int32)
        pix = None if pix_map is None else np.ascontiguousarray(pix_map, dtype=np.int32)
        if rows is not None and rows.size != m:
            raise KpdiError("row_map must have m entries")
        if k is None:
            k = exp.shape[1] if pix is None else pix.size
        if pix is not None and pix.size < k:
            raise KpdiError("pix_map must have at least k entries")
        md, err = C.c_float(0.0), C.c_int32(0)
        check(self._f.rescore_selftest(self._h, _ptr(exp), dtype_code(exp.dtype) if exp_dtype is None else int(exp_dtype),
                                       exp.shape[0], _ptr(rows), m, _ptr(dic),
                                       dtype_code(dic.dtype) if dict_dtype is None else int(dict_dtype), dic.shape[0],
                                       int(global_start), _ptr(pix), int(k), exp.shape[1], int(metric), _ptr(cs), _ptr(ci),
                                       stride, int(cand_offset), stride - int(cand_offset) if n_cand is None else int(n_cand),
                                       float(max_diff), _ptr(out), C.addressof(md), C.addressof(err)))
        return out, np.float32(md.value), err.value

    def fill_selftest(self, buffer, ranges):
        """merge.hip's fill_segments_kernel alone (kpdi_fill_selftest).  buffer: uint32 words; ranges: up to eight
        (byte_offset, words, value, bound_used).  Returns the buffer after the launch."""
        buf = np.array(buffer, dtype=np.uint32, order="C").ravel()
        off = np.array([r[0] for r in ranges], dtype=np.int64)
        words = np.array([r[1] for r in ranges], dtype=np.int64)
        value = np.array([r[2] for r in ranges], dtype=np.uint32)
        used = np.array([r[3] for r in ranges], dtype=np.int32)
        check(self._f.fill_selftest(self._h, len(ranges), _ptr(words), _ptr(value), _ptr(used), _ptr(off), _ptr(buf),
                                    buf.size))
        return buf

    # -- result consumers
    def orientation_similarity_map(self, simulation_indices, shape, keep_n, n_best, from_n_best, offsets,
                                   center_index, normalize):
        """simulation_indices: (ny * nx, keep_n) integers, or None = the lists resident from
        the last finalize().  offsets: (n_fp, 2) (dy, dx).  Returns (ny, nx, layers) float32."""
        ny, nx = shape
        idx = None
        if simulation_indices is not None:
            idx = np.ascontiguousarray(simulation_indices, dtype=np.int64).reshape(ny * nx, keep_n)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 2)
        out = np.empty((ny, nx, n_best - from_n_best + 1), dtype=np.float32)
        check(self._f.orientation_similarity_map(self._h, _ptr(idx), int(ny), int(nx), int(keep_n), int(n_best),
                                                     int(from_n_best), _ptr(off), off.shape[0], int(center_index),
                                                     int(bool(normalize)), _ptr(out)))
        return out

    def reset_topk(self):
        check(self._f.reset_topk(self._h))
        self._last_valid = False

    def holds_result(self, simulation_indices):
        """Whether `simulation_indices` (n, keep_n) are the lists the last finalize() returned
        (and that may therefore still be resident in HBM)."""
        if not self._last_valid:
            return False
        # what kpdi_finalize left in its page-locked staging buffer (no copy was kept: the caller may have masked or
        # remapped the array it got in place, and must then not be told that the device still holds "these" lists)
        p, n = C.POINTER(C.c_int32)(), C.c_int64(0)
        check(self._f.result_indices_i32(self._h, C.byref(p), C.byref(n)))
        idx = np.asarray(simulation_indices)
        if not p or n.value != idx.size:
            return False
        last = np.ctypeslib.as_array(p, shape=(n.value,))
        return bool(np.array_equal(idx.ravel(), last))

    def finalize(self, keep_n=None):
        """(scores (m, keep_n) float32 - float64 with COMPUTE_F64 -, indices (m, keep_n) int64).  `keep_n` must be the value
        last given to `set_problem` / `set_keep_n`: that is what the library writes."""
        if keep_n is None:
            keep_n = self._keep_n
        if self._keep_n is None or int(keep_n) != self._keep_n:
            raise KpdiError(f"finalize(keep_n={keep_n}) but the context keeps {self._keep_n} entries per pattern "
                            "(set_problem / set_keep_n)")
        if self._host_gather is not None:  # no usable RCCL communicator: the ranks' lists travel over the control plane
            self._host_gather.gather_lists(self)
        m = self.n_experimental
        indices = np.empty((m, keep_n), dtype=np.int64)
        if self._compute == COMPUTE_F64:  # float64 arithmetic: the rescored scores (csrc/rescore.hip)
            scores = np.empty((m, keep_n), dtype=np.float64)
            check(self._f.finalize_f64(self._h, _ptr(scores), _ptr(indices)))
        else:
            scores = np.empty((m, keep_n), dtype=np.float32)
            check(self._f.finalize(self._h, _ptr(scores), _ptr(indices)))
        self.result_token += 1
        self._last_valid = False
        self._check_filled(indices, keep_n)
        self._last_valid = self._compute != COMPUTE_F64
        return scores, indices

    @staticmethod
    def _check_filled(indices, keep_n):
        if indices.size and indices[:, -1].max() >= 2**31 - 1:  # unfilled entries rank last
            # unfilled list entries (index INT_MAX, score -inf): fewer than keep_n candidates ranked, which
            # only happens when scores are NaN (NaN / inf in the patterns) - the reference propagates
            # NaN there (out of contract); fail clearly instead of indexing with INT_MAX
            bad = np.flatnonzero((indices >= 2**31 - 1).any(axis=1))
            raise KpdiError(f"{bad.size} experimental pattern(s) (first: {bad[0]}) ranked fewer than {keep_n} "
                            "dictionary patterns: NaN scores (NaN or inf in the patterns?) or a dictionary "
                            "smaller than keep_n")

    def finalize_async(self, keep_n=None):
        """Queue the hand-over of the result (all-gather + merge over the ranks, device-to-host copies) and return a
        ticket at once; `finalize_wait(ticket)` collects it.  In between the NEXT map may already be queued
        (`set_experimental*`, `push_*`): a series of maps then never leaves the GPU idle during a hand-over."""
        if keep_n is None:
            keep_n = self._keep_n
        if self._keep_n is None or int(keep_n) != self._keep_n:
            raise KpdiError(f"finalize_async(keep_n={keep_n}) but the context keeps {self._keep_n} entries per pattern")
        if self._host_gather is not None:  # (the host-staged gather is synchronous; merge and hand-over still overlap)
            self._host_gather.gather_lists(self)
        t = C.c_int(-1)
        check(self._f.finalize_async(self._h, C.byref(t)))
        self.result_token += 1
        self._last_valid = False
        return (t.value, int(keep_n))

    def finalize_wait(self, ticket):
        """(scores (m, keep_n) float32, indices (m, keep_n) int64) of a `finalize_async` ticket."""
        slot, keep_n = ticket
        n = C.c_int64(0)
        check(self._f.pending_result_size(self._h, int(slot), C.byref(n)))
        m = n.value // keep_n
        scores = np.empty((m, keep_n), dtype=np.float32)
        indices = np.empty((m, keep_n), dtype=np.int64)
        check(self._f.finalize_wait(self._h, int(slot), _ptr(scores), _ptr(indices)))
        self._check_filled(indices, keep_n)
        return scores, indices

    # -- multi-GPU
    @staticmethod
    def comm_unique_id():
        buf = np.zeros(UNIQUE_ID_BYTES, dtype=np.uint8)
        check(load().kpdi_comm_unique_id(_ptr(buf)))
        return buf.tobytes()

    def comm_init(self, rank, nranks, unique_id):
        buf = np.frombuffer(unique_id, dtype=np.uint8).copy()
        if buf.size != UNIQUE_ID_BYTES:
            raise KpdiError("unique id must be 128 bytes")
        check(self._f.comm_init(self._h, int(rank), int(nranks), _ptr(buf)))
        self._has_comm = True  # (such an engine is never kept for another call: release_engine)

    def comm_selftest(self, n_bytes=1 << 20, timeout_ms=60000):
        """One all-gather of `n_bytes` per rank, awaited for at most `timeout_ms` (raises KpdiError otherwise)."""
        check(self._f.comm_selftest(self._h, int(n_bytes), int(timeout_ms)))

    def comm_drop(self):
        """Forget the RCCL communicator: `finalize` returns this context's own lists (or imported ones)."""
        check(self._f.comm_drop(self._h))

    def export_lists(self):
        """This context's OWN running best-k lists: (scores (m, keep_n) float32 / float64, indices (m, keep_n) int32)."""
        m = self.n_experimental
        scores = np.empty((m, self._keep_n), dtype=np.float64 if self._compute == COMPUTE_F64 else np.float32)
        indices = np.empty((m, self._keep_n), dtype=np.int32)
        check(self._f.export_lists(self._h, _ptr(scores), _ptr(indices)))
        return scores, indices

    def import_lists(self, scores_all, indices_all):
        """(n_ranks, m, keep_n) lists of all ranks: the next finalize merges THEM (host-staged gather)."""
        s = np.ascontiguousarray(scores_all, dtype=np.float64 if self._compute == COMPUTE_F64 else np.float32)
        i = np.ascontiguousarray(indices_all, dtype=np.int32)
        if s.shape != i.shape or s.ndim != 3 or s.shape[1:] != (self.n_experimental, self._keep_n):
            raise KpdiError(f"import_lists: lists of shape {s.shape} / {i.shape}, expected (n_ranks, {self.n_experimental}, {self._keep_n})")
        check(self._f.import_lists(self._h, _ptr(s), _ptr(i), s.shape[0]))

    # -- device buffers
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        check(self._f.dev_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def dev_free(self, d_ptr):
        check(self._f.dev_free(self._h, C.c_void_p(d_ptr)))

    def h2d(self, d_ptr, array):
        a = np.ascontiguousarray(array)
        check(self._f.h2d(self._h, C.c_void_p(d_ptr), _ptr(a), a.nbytes))

    def d2h(self, array, d_ptr):
        check(self._f.d2h(self._h, _ptr(array), C.c_void_p(d_ptr), array.nbytes))

    # -- measurement
    def set_profiling(self, on=True):
        """False / 0: off; True / 1: every phase of a sweep is bracketed by HIP events; "match" / 2: only the match
        launches (and the all-gather) are - an event record between two kernels idles the GPU for ~6 us."""
        check(self._f.set_profiling(self._h, {"match": 2, "epilogue": 3}.get(on, int(on) if not isinstance(on, str) else -1)))

    def counters(self):
        c = Counters()
        check(self._f.get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        check(self._f.reset_counters(self._h))


def resolve_devices(devices):
    """`devices=` of the host layer -> list of device ids, or None (= not given).
    "all": every visible GPU; an int: that many GPUs (0 .. n-1); a sequence of ids (an id may
    repeat: several members then share that GPU - the rehearsal form for 1-GPU hosts)."""
    if devices is None:
        return None
    if isinstance(devices, str):
        if devices.strip().lower() == "all":
            return list(range(max(device_count(), 1)))
        try:
            return [int(d) for d in devices.replace(",", " ").split()]
        except ValueError:
            raise KpdiError(f"devices={devices!r}: expected 'all' or a list of device ids") from None
    if isinstance(devices, (int, np.integer)):
        if devices < 1:
            raise KpdiError("devices must name at least one GPU")
        return list(range(int(devices)))
    out = [int(d) for d in devices]
    if not out:
        raise KpdiError("devices must name at least one GPU")
    return out


LAUNCHER_VARIABLES = ("WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID", "SLURM_LOCALID", "OMPI_COMM_WORLD_RANK", "PMI_RANK")
_logged_defaults = set()


def under_a_launcher():
    """A launcher that starts one process per GPU (torchrun, srun, mpirun) has exported its variables: such a process
    must not spread over every GPU by itself - its siblings would all do the same."""
    return any(v in os.environ for v in LAUNCHER_VARIABLES)


def default_devices():
    """What a call that says nothing about devices runs on: $KPDI_DEVICES ("all" or ids like "0,1,2") if set; else, in a
    process started by a launcher (`under_a_launcher`), ONE GPU - the process's local rank ($LOCAL_RANK /
    $SLURM_LOCALID modulo the visible devices); else every visible GPU - the counterpart of the reference using every
    core of the host (its Dask scheduler's default).  What was chosen is logged once per choice
    (`logging.getLogger("kikuchipy_amd")`, level INFO)."""
    env = os.environ.get("KPDI_DEVICES")
    if env:
        ids, why = resolve_devices(env), f"$KPDI_DEVICES={env}"
    elif under_a_launcher():
        local = os.environ.get("LOCAL_RANK") or os.environ.get("SLURM_LOCALID") or "0"
        n = max(device_count(), 1)
        ids = [int(local) % n if local.lstrip("-").isdigit() else 0]
        why = ("a launcher's environment (" + ", ".join(v for v in LAUNCHER_VARIABLES if v in os.environ) +
               "): one process per GPU is assumed; name devices= or set $KPDI_DEVICES to override")
    else:
        ids, why = resolve_devices("all"), "every visible GPU"
    key = (tuple(ids), why)
    if key not in _logged_defaults:
        _logged_defaults.add(key)
        import logging

        logging.getLogger("kikuchipy_amd").info("no device named: running on GPU(s) %s (%s)", ids, why)
    return ids


def make_engine(device=0, devices=None, gather=None):
    """A `Context` on one GPU, or - for more than one device id - a `Group` over them."""
    ids = resolve_devices(devices)
    if ids is None:
        return Context(device)
    if len(ids) == 1 and gather is None:
        return Context(ids[0])
    return Group(ids, gather=gather)


# ---- engines that outlive the call that made them --------------------------------------------------------------------
# `kikuchipy_amd.dictionary_indexing(..., metric="ncc")` makes its own engine.  Creating one (context, streams, the first
# allocation of the prepared matrices and staging buffers) and destroying it (hipFree synchronises) was 6-7 ms of every
# such call - a quarter of a 30 ms call at configs[1].  The engine of a finished call is therefore kept, idle, ONE per set
# of devices, and handed to the next call that names the same devices (its device buffers stay allocated: they are sized
# for the job before).  `clear_engine_cache()` closes them; KPDI_ENGINE_CACHE=0 switches the cache off.
_ENGINE_POOL = {}
_ENGINE_POOL_LOCK = threading.Lock()


def _engine_key(device, devices, gather):
    ids = resolve_devices(devices)
    return (tuple(ids) if ids is not None else (int(device),), gather)


def acquire_engine(device=0, devices=None, gather=None):
    """`make_engine`, or the idle engine an earlier call released for the same devices."""
    key = _engine_key(device, devices, gather)
    engine = None
    if os.environ.get("KPDI_ENGINE_CACHE", "1") != "0":
        with _ENGINE_POOL_LOCK:
            engine = _ENGINE_POOL.pop(key, None)
    if engine is not None and hasattr(engine, "_h") and not (engine._h and engine._h.value):
        engine = None  # (closed behind the pool's back)
    if engine is None:
        engine = make_engine(device, devices, gather)
    engine._pool_key = key
    return engine


def release_engine(engine):
    """The call that acquired `engine` has finished with it, successfully: keep it for the next one (held chunks
    released, profiling off), or close it when the cache is off, holds one already, or the engine was given a
    communicator (that belongs to the job that attached it)."""
    key = getattr(engine, "_pool_key", None)
    keep = key is not None and os.environ.get("KPDI_ENGINE_CACHE", "1") != "0" and getattr(engine, "_host_gather", None) is None \
        and not getattr(engine, "_has_comm", False)
    if keep:
        try:
            if hasattr(engine, "release_held"):
                engine.release_held()
            engine.set_profiling(False)
            engine.reset_counters()  # (the next call's counters are its own)
            getattr(engine, "_keep", {}).clear()
            with _ENGINE_POOL_LOCK:
                if key not in _ENGINE_POOL:
                    _ENGINE_POOL[key] = engine
                    return
        except Exception:  # noqa: BLE001 - an engine that cannot be tidied up is not kept
            pass
    engine.close()


def clear_engine_cache():
    """Close the idle engines `dictionary_indexing` calls left behind (and free their device memory)."""
    with _ENGINE_POOL_LOCK:
        engines = list(_ENGINE_POOL.values())
        _ENGINE_POOL.clear()
    for e in engines:
        try:
            e.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


atexit.register(clear_engine_cache)


class Group(Context):
    """Several GPUs behind the interface of one `Context` (`kpdi_group`, include/kpdi.h): the
    experimental set is replicated, every dictionary chunk is block-assigned to the members,
    `finalize()` returns the one merged result.  One Python thread drives it; the members' host
    work runs on the library's own threads.

    A `Context` method does one of three things here.  With a group form of every symbol it calls it is inherited
    and runs on all members (`self._f.X` is `kpdi_group_X`), unless the class overrides it by hand.  Named in
    `_ON_ROOT` it runs on member 0.  Named in `_ONE_GPU` it raises `KpdiError`: use `group.members[i]`.

    gather: None (automatic: RCCL when the devices are distinct, peer copies otherwise,
    $KPDI_GATHER overrides), "rccl" or "p2p"."""

    _prefix = "kpdi_group_"
    _GATHER = {None: GATHER_AUTO, "auto": GATHER_AUTO, "rccl": GATHER_RCCL, "p2p": GATHER_P2P}
    # calls without a group form that run on member 0: every member holds the same patterns and master pattern, and the
    # merged lists of the last finalize live there
    _ON_ROOT = ("get_direction_cosines", "project_patterns", "project_patterns_varying_pc", "refine_set_patterns",
                "refine_get_prepared", "refine_objective", "refine_solve", "nelder_mead_selftest", "refine_solve_powell",
                "powell_selftest", "refine_solve_nlopt", "nlopt_simplex_selftest", "refine_solve_de", "de_selftest",
                "mt19937_selftest", "orientation_similarity_map", "kinematical_master_pattern", "sample_fundamental",
                "orientation_pairs", "orientation_outer", "orientation_reduce", "orientation_kam", "geometrical_visibility",
                "geometrical_coordinates")
    # calls that belong to one GPU (its resident patterns, its device buffers) or to one rank: refused on a group
    _ONE_GPU = ("image_quality", "region_sums", "reduce", "fft_filter", "rescale_intensity", "normalize_intensity",
                "intensity_range", "adaptive_histogram_equalization", "downsample", "get_dynamic_background", "change_dtype",
                "select_patterns", "set_navigation_mask", "decomposition_gram", "decomposition_apply", "decomposition_model",
                "hough_bands", "hough_index", "average_neighbour_patterns", "neighbour_dot_products", "merge_selftest",
                "merge64_selftest", "rescore_selftest", "fill_selftest", "comm_selftest", "comm_drop", "export_lists",
                "import_lists", "dev_alloc", "dev_free", "h2d", "d2h", "comm_init")

    def __init__(self, devices="all", gather=None):
        ids = resolve_devices(devices)
        if gather not in self._GATHER:
            raise KpdiError(f"gather must be None, 'rccl' or 'p2p', not {gather!r}")
        self._f = _Functions(self._prefix)
        self._owned = True
        self._h = C.c_void_p()
        arr = (C.c_int * len(ids))(*ids)
        check(self._f.create(arr, len(ids), self._GATHER[gather], C.byref(self._h)))
        self.devices = list(ids)
        self.device = ids[0]
        self.members = [Context(d, _borrowed=self._f.member(self._h, i)) for i, d in enumerate(ids)]
        self.root = self.members[0]
        self._init_state()
        self._borrowed = []  # (ticket, array): host chunks the members' uploads may still be reading

    def __len__(self):
        return len(self.devices)

    @property
    def gather(self):
        """"rccl", "p2p" or "none" (one device): how the members' lists reach member 0."""
        return GATHER_NAMES[int(self._f.gather(self._h))]

    def describe(self):
        return (self._f.describe(self._h) or b"").decode()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for m in self.members:
                m._h = C.c_void_p()
            self._f.destroy(self._h)  # (joins the members' threads: nothing reads a borrowed chunk afterwards)
            self._h = C.c_void_p()
            self._borrowed = []

    @staticmethod
    def chunk_share(n_chunk, i, n_dev):
        """Rows [start, end) of the `i`-th of `n_dev` near-equal contiguous parts of `n_chunk` rows (a member's quota)."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(load().kpdi_group_chunk_share(int(n_chunk), int(i), int(n_dev), C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def assign_chunk(n_dev, n_total, loads, n_chunk, min_piece=1):
        """The library's chunk assignment (csrc/group_assign.h) as a pure function: [(member, first row, rows), ...]
        for a chunk of `n_chunk` patterns; `loads` (list, one entry per member) is updated in place."""
        ld = (C.c_int64 * n_dev)(*[int(v) for v in loads])
        cap = n_dev + 1
        mem, row0, rows, n = (C.c_int * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int(0)
        check(load().kpdi_group_assign_chunk(int(n_dev), int(n_total), int(min_piece), ld, int(n_chunk), cap, mem, row0,
                                             rows, C.byref(n)))
        loads[:] = list(ld)
        return [(mem[i], row0[i], rows[i]) for i in range(n.value)]

    def set_dictionary_size(self, n_total):
        check(self._f.set_dictionary_size(self._h, int(n_total)))

    def push_dictionary_chunk(self, patterns, global_start):
        """Queue the chunk on the member(s) that take it and return: the array is borrowed by the library (and kept
        alive here) until the members' uploads have read it."""
        p = np.ascontiguousarray(patterns)
        t = C.c_int64(0)
        check(self._f.push_dictionary_chunk_borrowed(self._h, _ptr(p), dtype_code(p.dtype), p.shape[0], int(global_start),
                                                     C.byref(t)))
        self._borrowed.append((t.value, p))
        self._drop_consumed()

    def _drop_consumed(self, everything=False):
        if everything:
            self._borrowed.clear()
        elif self._borrowed:
            t = C.c_int64(0)
            check(self._f.chunks_consumed(self._h, C.byref(t)))
            self._borrowed = [(k, a) for k, a in self._borrowed if k > t.value]

    def synchronize(self):
        super().synchronize()
        self._drop_consumed(True)

    def _after_finalize(self, ok):
        """Borrowed host chunks after a finalize: the C call joins its members' host work before anything is gathered, so
        after a SUCCESSFUL return every chunk has been read and all may go.  After an exception the call may have failed
        before that join (a Python-side check, an allocation): queued uploads may still be reading the arrays - only what
        the library reports as consumed is dropped (use-after-free otherwise)."""
        if ok:
            self._drop_consumed(True)
            return
        try:
            self._drop_consumed()
        except KpdiError:
            pass

    def finalize(self, keep_n=None):
        ok = False
        try:
            res = super().finalize(keep_n)
            ok = True
            return res
        finally:
            self._after_finalize(ok)

    def finalize_async(self, keep_n=None):
        ok = False
        try:
            res = super().finalize_async(keep_n)
            ok = True
            return res
        finally:
            self._after_finalize(ok)

    # -- what differs from a single context
    def set_problem(self, sy, sx, signal_mask=None, metric=METRIC_NCC, keep_n=20, compute=COMPUTE_F32):
        super().set_problem(sy, sx, signal_mask, metric, keep_n, compute)
        for m in self.members:
            m._keep_n, m._compute = self._keep_n, self._compute

    def set_keep_n(self, keep_n):
        super().set_keep_n(keep_n)
        for m in self.members:
            m._keep_n = self._keep_n

    def set_experimental(self, patterns, navigation_mask=None):
        p = np.ascontiguousarray(patterns)
        nm = _mask_bytes(navigation_mask)
        if nm is not None and nm.size != p.shape[0]:
            raise KpdiError(f"navigation mask has {nm.size} elements, there are {p.shape[0]} patterns")
        # (returns when every member's upload has consumed `p`)
        check(self._f.set_experimental(self._h, _ptr(p), dtype_code(p.dtype), p.shape[0], _ptr(nm)))
        self._exp_shape, self._exp_dtype = p.shape, p.dtype

    def set_experimental_h5ebsd(self, path, scan=None, navigation_mask=None):
        info, pats, _, _ = h5ebsd_read(path, scan)
        self.set_experimental(pats.reshape((-1,) + pats.shape[-2:]), navigation_mask)
        return info

    def set_experimental_dev(self, d_ptrs, dtype, m_all, navigation_mask=None):
        """d_ptrs: one device pointer per member (the set in that member's HBM)."""
        if len(d_ptrs) != len(self.members):
            raise KpdiError(f"{len(d_ptrs)} device pointers for {len(self.members)} members")
        nm = _mask_bytes(navigation_mask)
        arr = (C.c_void_p * len(d_ptrs))(*[int(p) for p in d_ptrs])
        check(self._f.set_experimental_dev(self._h, arr, dtype_code(dtype), int(m_all), _ptr(nm)))
        self._record_experimental_dev(dtype, m_all)

    def push_dictionary_chunk_dev(self, d_ptrs, dtype, n_chunk, global_start):
        """One device chunk per member: d_ptrs[i], n_chunk[i] patterns (0 = none), first dictionary
        index global_start[i]."""
        n = len(self.members)
        if not (len(d_ptrs) == len(n_chunk) == len(global_start) == n):
            raise KpdiError(f"push_dictionary_chunk_dev needs one entry per member ({n})")
        ptrs = (C.c_void_p * n)(*[int(p) if p else None for p in d_ptrs])
        cnt = (C.c_int64 * n)(*[int(v) for v in n_chunk])
        st = (C.c_int64 * n)(*[int(v) for v in global_start])
        check(self._f.push_dictionary_chunk_dev(self._h, ptrs, dtype_code(dtype), cnt, st))

    def hold_dictionary_chunk_dev(self, d_ptrs, dtype, n_chunk, global_start):
        for m, p, n, s0 in zip(self.members, d_ptrs, n_chunk, global_start):
            if n > 0:
                m.hold_dictionary_chunk_dev(p, dtype, n, s0)

    def set_direction_cosines(self, direction_cosines):
        for m in self.members:
            m.set_direction_cosines(direction_cosines)
        self._projection_key = None
        self._dc_npix = self.root._dc_npix

    def set_detector(self, gnomonic_bounds, pcz, nrows, ncols, om_detector_to_sample):
        super().set_detector(gnomonic_bounds, pcz, nrows, ncols, om_detector_to_sample)
        self.root._dc_npix = self._dc_npix

    def push_rotations_chunk_varying_pc(self, rotations, pcs, global_start, om_detector_to_sample, rescale=False,
                                        out_min=-1.0, out_max=1.0):
        """One contiguous block of the chunk per member (the members' queues are joined first: this path drives the member
        contexts from the caller's thread)."""
        rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        pc = np.ascontiguousarray(pcs, dtype=np.float64).reshape(-1, 3)
        self.synchronize()
        for i, m in enumerate(self.members):
            a, b = self.chunk_share(rot.shape[0], i, len(self.members))
            if b > a:
                m.push_rotations_chunk_varying_pc(rot[a:b], pc[a:b], global_start + a, om_detector_to_sample, rescale, out_min, out_max)

    def holds_result(self, simulation_indices):
        self.root._last_valid = self._last_valid
        return self.root.holds_result(simulation_indices)

    # the two calls of the basinhopping solver have no group form and run on member 0, like the calls of `_ON_ROOT`
    def refine_solve_basinhopping(self, *args, **kwargs):
        return self.root.refine_solve_basinhopping(*args, **kwargs)

    def basinhopping_selftest(self, *args, **kwargs):
        return self.root.basinhopping_selftest(*args, **kwargs)

    # belongs to one GPU like the calls of `_ONE_GPU`, next to `hough_index` there: refused on a group
    def hough_optimize_pc(self, *args, **kwargs):
        raise KpdiError("hough_optimize_pc works on one GPU's own state or buffers and has no group form: use "
                        "group.members[i].hough_optimize_pc(...)")

    # -- measurement
    def counters(self):
        """Member 0's counters (its merge / gather figures are the group's) + `members`: every member's."""
        per = [m.counters() for m in self.members]
        out = dict(per[0])
        out["members"] = per
        out["gather"] = self.gather
        return out


def _on_root(name):
    def method(self, *args, **kwargs):
        return getattr(self.root, name)(*args, **kwargs)
    return method


def _one_gpu(name):
    def method(self, *args, **kwargs):
        if name == "comm_init":
            raise KpdiError("comm_init: a Group gathers inside one process; ranks of a multi-process job attach a "
                            "Context each (group.members[i] is one)")
        raise KpdiError(f"{name} works on one GPU's own state or buffers and has no group form: use "
                        f"group.members[i].{name}(...)")
    return method


for _make, _names in ((_on_root, Group._ON_ROOT), (_one_gpu, Group._ONE_GPU)):
    for _name in _names:
        _method = _make(_name)
        _method.__name__, _method.__doc__ = _name, getattr(Context, _name).__doc__
        setattr(Group, _name, _method)
for _name in ("refine_solve_basinhopping", "basinhopping_selftest", "hough_optimize_pc"):
    getattr(Group, _name).__doc__ = getattr(Context, _name).__doc__
