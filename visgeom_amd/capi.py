"""ctypes binding of include/visgeom_amd.h (the C ABI is the product boundary; this file is plumbing).

The library is HIP-only.  If it has not been built this module raises -- it never falls back to
a CPU implementation."""
import ctypes
import os

from . import _build

_dp = ctypes.POINTER(ctypes.c_double)
_dpp = ctypes.POINTER(_dp)
_ip = ctypes.POINTER(ctypes.c_int)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p
_vpp = ctypes.POINTER(ctypes.c_void_p)

MODEL_EUCM, MODEL_UCM, MODEL_MEI = 0, 1, 2
MODEL_KB, MODEL_DS = 4, 5   # Kannala-Brandt and double sphere (not in the reference); 3 is unassigned and refused
MODELS = {"eucm": MODEL_EUCM, "ucm": MODEL_UCM, "mei": MODEL_MEI, "kb": MODEL_KB, "ds": MODEL_DS}
NUM_INTRINSICS = {MODEL_EUCM: 6, MODEL_UCM: 5, MODEL_MEI: 10, MODEL_KB: 8, MODEL_DS: 6}
TRANSFORM_DIRECT, TRANSFORM_INVERSE = 0, 1
MAX_CHAIN = 5
DOUBLE_BIG = 1e15
OK = 0
ERR_INVALID_ARGUMENT, ERR_HIP, ERR_NO_DEVICE, ERR_STATE, ERR_ALLOC, ERR_NUMERIC = 1, 2, 3, 4, 5, 6
PIXEL_U8, PIXEL_F32 = 0, 1

ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, _dp, ctypes.c_int64, ctypes.c_void_p)


class SolveOptions(ctypes.Structure):
    """struct vg_solve_options"""
    _fields_ = [("max_num_iterations", ctypes.c_int), ("function_tolerance", ctypes.c_double),
                ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("initial_trust_region_radius", ctypes.c_double), ("max_trust_region_radius", ctypes.c_double),
                ("min_trust_region_radius", ctypes.c_double), ("min_relative_decrease", ctypes.c_double),
                ("min_lm_diagonal", ctypes.c_double), ("max_lm_diagonal", ctypes.c_double),
                ("use_bounds", ctypes.c_int), ("verbose", ctypes.c_int), ("soft_l1_scale", ctypes.c_double),
                ("allreduce", ALLREDUCE_FN), ("allreduce_user", ctypes.c_void_p), ("comm", ctypes.c_void_p)]


class DatasetOutputs(ctypes.Structure):
    """struct vg_dataset_outputs"""
    _fields_ = [("residuals", ctypes.c_void_p), ("jac_intr", ctypes.c_void_p), ("jac_member", ctypes.c_void_p * MAX_CHAIN)]


class SolveSummary(ctypes.Structure):
    """struct vg_solve_summary"""
    _fields_ = [("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("num_iterations", ctypes.c_int), ("num_successful_steps", ctypes.c_int), ("termination", ctypes.c_int),
                ("gradient_max_norm", ctypes.c_double), ("final_radius", ctypes.c_double),
                ("total_seconds", ctypes.c_double), ("evaluate_seconds", ctypes.c_double),
                ("schur_seconds", ctypes.c_double), ("host_seconds", ctypes.c_double),
                ("num_global_columns", ctypes.c_int), ("num_pose_blocks", ctypes.c_int64),
                ("message", ctypes.c_char * 160)]


class CalibrationTimings(ctypes.Structure):
    """struct vg_calibration_timings"""
    _fields_ = [(n, ctypes.c_double) for n in ("read_files_s", "parse_json_s", "geometric_init_s", "refine_total_s", "refine_kernel_s",
                                               "global_init_s", "assemble_s", "solve_s", "readback_s", "residual_eval_s",
                                               "residual_format_s")] + \
               [(n, ctypes.c_int64) for n in ("refine_images", "refine_iterations", "refine_max_iterations", "json_bytes", "residual_lines")] + \
               [("corner_upload_s", ctypes.c_double), ("corner_uploads", ctypes.c_int64), ("corner_upload_bytes", ctypes.c_int64)]


TERMINATION = {0: "CONVERGENCE_FUNCTION", 1: "CONVERGENCE_GRADIENT", 2: "CONVERGENCE_PARAMETER", 3: "NO_CONVERGENCE",
               4: "RADIUS_TOO_SMALL", 5: "FAILURE"}

# every symbol include/visgeom_amd.h declares: (restype, argtypes)
SIGNATURES = {
    "vg_abi_version": (ctypes.c_int, []),
    "vg_last_error": (ctypes.c_char_p, []),
    "vg_device_count": (ctypes.c_int, []),
    "vg_num_intrinsics": (ctypes.c_int, [ctypes.c_int]),
    "vg_intrinsic_bounds": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _dp, _dp]),
    "vg_block_create": (ctypes.c_int, [_vpp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ip, ctypes.c_int, _dp, _dp]),
    "vg_block_num_residuals": (ctypes.c_int, [_vp]),
    "vg_block_num_parameter_blocks": (ctypes.c_int, [_vp]),
    "vg_block_parameter_block_size": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_block_evaluate": (ctypes.c_int, [_vp, _dpp, _dp, _dpp]),
    "vg_block_destroy": (None, [_vp]),
    "vg_block_group_create": (ctypes.c_int, [_vpp, ctypes.c_int, ctypes.c_int]),
    "vg_block_create_in_group": (ctypes.c_int, [_vpp, _vp, ctypes.c_int, ctypes.c_int, _ip, ctypes.c_int, _dp, _dp]),
    "vg_block_group_invalidate": (ctypes.c_int, [_vp]),
    "vg_block_group_stats": (ctypes.c_int, [_vp, _i64p, _i64p, _i64p, _i64p]),
    "vg_block_group_destroy": (None, [_vp]),
    "vg_problem_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp]),
    "vg_problem_destroy": (None, [_vp]),
    "vg_problem_add_camera": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, _ip]),
    "vg_problem_add_transform": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _ip]),
    "vg_problem_add_dataset": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _ip, _ip, ctypes.c_int, _dp,
                                              ctypes.c_int64, _i32p, _dp, _ip]),
    "vg_problem_add_transformation_prior": (ctypes.c_int, [_vp, ctypes.c_int, _dp]),
    "vg_problem_add_odometry_prior": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                                     ctypes.c_double, _dp, _dp]),
    "vg_problem_add_parameter_block": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.c_int, _ip]),
    "vg_problem_parameter_block_offset": (ctypes.c_int64, [_vp, ctypes.c_int]),
    "vg_problem_add_odometry_cost": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                                    ctypes.c_double, ctypes.c_int, _dp, ctypes.c_int]),
    "vg_odometry_cost_evaluate": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, _dp, _dp, _dp,
                                                 _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "vg_odometry_prior_evaluate": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _dp, _dp,
                                                  _dp, _dp]),
    "vg_problem_set_pose_constant": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64]),
    "vg_problem_finalize": (ctypes.c_int, [_vp]),
    "vg_problem_num_parameters": (ctypes.c_int64, [_vp]),
    "vg_problem_camera_offset": (ctypes.c_int64, [_vp, ctypes.c_int]),
    "vg_problem_transform_offset": (ctypes.c_int64, [_vp, ctypes.c_int, ctypes.c_int64]),
    "vg_problem_set_parameters": (ctypes.c_int, [_vp, _dp]),
    "vg_problem_get_parameters": (ctypes.c_int, [_vp, _dp]),
    "vg_problem_parameters_device": (_vp, [_vp]),
    "vg_problem_num_datasets": (ctypes.c_int, [_vp]),
    "vg_dataset_num_blocks": (ctypes.c_int64, [_vp, ctypes.c_int]),
    "vg_dataset_num_points": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_dataset_chain_len": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_dataset_single_launch": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_dataset_num_intrinsics": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_problem_prepare": (ctypes.c_int, [_vp]),
    "vg_problem_force_prepared_frames": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_dataset_evaluate": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vpp]),
    "vg_problem_evaluate": (ctypes.c_int, [_vp, ctypes.POINTER(DatasetOutputs)]),
    "vg_problem_synchronize": (ctypes.c_int, [_vp]),
    "vg_dataset_evaluate_to_host": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vpp]),
    "vg_dataset_failed_count": (ctypes.c_int, [_vp, ctypes.c_int, _i64p]),
    "vg_dataset_gram_width": (ctypes.c_int, [_vp, ctypes.c_int]),
    "vg_dataset_gram_fused": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "vg_problem_gram_fused": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_void_p)]),
    "vg_problem_gram_fused_sum": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "vg_dataset_gram_fused_sum": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    "vg_dataset_gram_from_rows": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vpp, _vp]),
    "vg_dataset_gram_sum": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    "vg_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "vg_comm_create": (ctypes.c_int, [_vpp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vg_comm_adopt": (ctypes.c_int, [_vpp, _vp, ctypes.c_int]),
    "vg_comm_create_replicated": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "vg_comm_create_local": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    "vg_comm_size": (ctypes.c_int, [_vp]),
    "vg_comm_rank": (ctypes.c_int, [_vp]),
    "vg_comm_allreduce_sum": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp]),
    "vg_comm_destroy": (None, [_vp]),
    "vg_solve_options_init": (None, [ctypes.POINTER(SolveOptions)]),
    "vg_release_cached_memory": (None, []),
    "vg_problem_solve": (ctypes.c_int, [_vp, ctypes.POINTER(SolveOptions), ctypes.POINTER(SolveSummary)]),
    "vg_refine_poses": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, ctypes.c_int, _dp, ctypes.c_int64, _dp, _dp,
                                       ctypes.POINTER(SolveOptions), _i32p, _dp, _i32p]),
    "vg_refine_poses_timed": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, ctypes.c_int, _dp, ctypes.c_int64, _dp, _dp,
                                             ctypes.POINTER(SolveOptions), _i32p, _dp, _i32p, _dp]),
    "vg_dataset_refine_poses": (ctypes.c_int, [_vp, ctypes.c_int, _dp, ctypes.POINTER(SolveOptions), _i32p, _dp, _i32p, _dp]),
    "vg_host_cholesky_solve": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp]),
    "vg_calibration_create": (ctypes.c_int, [_vpp, ctypes.c_int]),
    "vg_calibration_destroy": (None, [_vp]),
    "vg_calibration_add_file": (ctypes.c_int, [_vp, ctypes.c_char_p]),
    "vg_calibration_compute": (ctypes.c_int, [_vp, ctypes.POINTER(SolveOptions), ctypes.POINTER(SolveSummary)]),
    "vg_calibration_report": (ctypes.c_int64, [_vp, ctypes.c_char_p, ctypes.c_int64]),
    "vg_calibration_log": (ctypes.c_int64, [_vp, ctypes.c_char_p, ctypes.c_int64]),
    "vg_calibration_num_datasets": (ctypes.c_int, [_vp]),
    "vg_calibration_get_intrinsics": (ctypes.c_int, [_vp, ctypes.c_char_p, _dp, _ip]),
    "vg_calibration_get_transform": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int64, _dp, _i64p]),
    "vg_calibration_write_residuals": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_char_p, _dp, _i64p]),
    "vg_calibration_get_corners": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _dp, _i64p]),
    "vg_calibration_num_images": (ctypes.c_int64, [_vp, ctypes.c_int]),
    "vg_calibration_get_timings": (ctypes.c_int, [_vp, ctypes.POINTER(CalibrationTimings)]),
    "vg_reconstruct_point": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp]),
    "vg_initial_grid_pose": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp]),
    "vg_init_transform": (ctypes.c_int, [ctypes.c_int, _ip, ctypes.c_int, _dp, _dp, _dp]),
    "vg_init_transform_range": (ctypes.c_int, [ctypes.c_int, _ip, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp]),
    "vg_transform_from_values": (ctypes.c_int, [ctypes.c_int, _dp, _dp]),
    "vg_sparse_reproject_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, ctypes.c_int, _dp, _dp, ctypes.c_int64, _i64p, _dp, _dp, _dp, _dp]),
    "vg_mono_reproject_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, ctypes.c_int, _dp, _dp, ctypes.c_int64, _dp, _dp]),
    "vg_reproject_num_blocks": (ctypes.c_int64, [_vp]),
    "vg_reproject_num_points": (ctypes.c_int64, [_vp]),
    "vg_reproject_block_offset": (ctypes.c_int64, [_vp, ctypes.c_int64]),
    "vg_sparse_reproject_evaluate": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "vg_mono_reproject_evaluate": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "vg_sparse_reproject_block_evaluate": (ctypes.c_int, [_vp, ctypes.c_int64, _dpp, _dp, _dpp]),
    "vg_mono_reproject_block_evaluate": (ctypes.c_int, [_vp, ctypes.c_int64, _dpp, _dp, _dpp]),
    "vg_reproject_synchronize": (ctypes.c_int, [_vp]),
    "vg_reproject_destroy": (None, [_vp]),
    "vg_camera_jacobian_evaluate": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, _dp, _dp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "vg_rectify_map": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, _dp, _dp, _vp, _vp]),
    "vg_remap": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp,
                                ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_double, _vp]),
    "vg_corner_detector_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vg_corner_detector_destroy": (None, [_vp]),
    "vg_corner_detect": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, _dp, _vp, _dp]),
    "vg_corner_response": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_double, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _dp]),
    "vg_corner_candidates": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_int,
                                            _i32p, _i32p, _dp, _i64p]),
    "vg_corner_circle": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i32p, _i32p, _ip]),
    "vg_corner_detector_stats": (ctypes.c_int, [_vp, _dp]),
    "vg_corner_detector_chunk": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _ip]),
    "vg_stereo_params_default": (None, [_vp]),
    "vg_stereo_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _dp, _dp, _vp]),
    "vg_stereo_destroy": (None, [_vp]),
    "vg_stereo_size": (ctypes.c_int, [_vp, _ip, _ip]),
    "vg_stereo_chunk": (ctypes.c_int, [_vp, _i64p]),
    "vg_stereo_compute": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vg_stereo_compute_mh": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "vg_stereo_geometry": (ctypes.c_int, [_vp, _vp]),
    "vg_stereo_curve_cost": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vg_stereo_aggregate": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "vg_stereo_curve_walk": (ctypes.c_int, [_dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            _i32p]),
    "vg_motion_stereo_params_default": (None, [_vp]),
    "vg_motion_stereo_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _dp, _vp]),
    "vg_motion_stereo_destroy": (None, [_vp]),
    "vg_motion_stereo_size": (ctypes.c_int, [_vp, _ip, _ip]),
    "vg_motion_stereo_set_base": (ctypes.c_int, [_vp, ctypes.c_int64, _vp]),
    "vg_motion_stereo_compute": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64p]),
    "vg_motion_stereo_mask": (ctypes.c_int, [_vp, _vp]),
    "vg_motion_stereo_select": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp, _vp, _vp, _vp, _vp]),
    "vg_depth_fusion_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _vp]),
    "vg_depth_fusion_destroy": (None, [_vp]),
    "vg_depth_fusion_size": (ctypes.c_int, [_vp, _ip, _ip]),
    "vg_depth_warp": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _i64p]),
    "vg_depth_merge": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _i64p]),
    "vg_depth_filter_noise": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _i64p]),
    "vg_depth_regularize": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp]),
    "vg_depth_pack_mh": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _i64p, _vp, _vp, _vp, _vp]),
    "vg_depth_reconstruct": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, _vp, _vp, ctypes.c_int64, _vp, _vp, _dp, _i64p, _vp]),
    "vg_depth_generate_plane": (ctypes.c_int, [_vp, _dp, ctypes.c_int, _dp, _vp, _vp, _vp]),
    "vg_depth_compare": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_double, _i64p, _dp, _vp]),
    "vg_transform_inverse": (ctypes.c_int, [_dp, _dp]),
    "vg_transform_inverse_compose": (ctypes.c_int, [_dp, _dp, _dp]),
    "vg_photometric_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _vp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vg_photometric_destroy": (None, [_vp]),
    "vg_photometric_level_size": (ctypes.c_int, [_vp, ctypes.c_int, _ip, _ip]),
    "vg_photometric_set_base": (ctypes.c_int, [_vp, _vp, _vp]),
    "vg_photo_set_depth": (ctypes.c_int, [_vp, _vp]),
    "vg_photometric_set_targets": (ctypes.c_int, [_vp, ctypes.c_int64, _vp]),
    "vg_photometric_level": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp]),
    "vg_photometric_pack": (ctypes.c_int, [_vp, ctypes.c_int, _i64p, _vp, _vp, _vp]),
    "vg_photometric_evaluate": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _dp, _i32p, _vp, _vp, _dp, _dp, _dp]),
    "vg_photometric_compute_pose": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _i32p, _dp, _dp, _dp]),
    "vg_mi_evaluate": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _dp, _i32p, _vp, _dp, _dp, _dp]),
    "vg_mi_compute_pose": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _i32p, _dp, _vp, _dp, _dp]),
    "vg_mi_odometry": (ctypes.c_int, [_dp, _dp, _dp, _dp, _dp]),
    "vg_sparse_odom_params_default": (None, [_vp]),
    "vg_sparse_odom_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _dp, ctypes.c_int, ctypes.c_int, _vp]),
    "vg_sparse_odom_destroy": (None, [_vp]),
    "vg_sparse_odom_response": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp]),
    "vg_sparse_odom_detect": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _i32p, _vp, _vp]),
    "vg_sparse_odom_match": (ctypes.c_int, [_vp, ctypes.c_int64, _i32p, _vp, _i32p, _vp, _i32p, _vp, _vp]),
    "vg_sparse_odom_solve": (ctypes.c_int, [_vp, ctypes.c_int64, _i64p, _vp, _vp, _vp, _vp, _dp, _dp, _dp]),
    "vg_sparse_odom_score": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, ctypes.c_int64, _vp, _vp, _vp, _vp, _i32p]),
    "vg_sparse_odom_draw_samples": (ctypes.c_int, [_vp, ctypes.c_int64, _i32p]),
    "vg_sparse_odom_ransac": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _dp, _i32p, _dp, _vp, _dp]),
    "vg_sparse_odom_feed": (ctypes.c_int, [_vp, _vp, _dp, _i32p, _dp, _dp]),
    "vg_sparse_odom_increment": (ctypes.c_int, [_vp, _dp]),
    "vg_sparse_odom_integrated": (ctypes.c_int, [_vp, _dp]),
    "vg_render_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "vg_render_destroy": (None, [_vp]),
    "vg_render_size": (ctypes.c_int, [_vp, _ip, _ip]),
    "vg_render_set_camera": (ctypes.c_int, [_vp, _dp]),
    "vg_render_views": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp, _vp, _vp, _vp, _vp, _i64p]),
    "vg_render_filter_kernel": (ctypes.c_int, [ctypes.c_int, _dp]),
    "vg_mono_odom_params_default": (None, [_vp]),
    "vg_mono_odom_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _dp, ctypes.c_int, ctypes.c_int, _vp]),
    "vg_mono_odom_destroy": (None, [_vp]),
    "vg_mono_odom_size": (ctypes.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "vg_mono_odom_feed_wheel_odometry": (ctypes.c_int, [_vp, _dp]),
    "vg_mono_odom_feed_image": (ctypes.c_int, [_vp, _vp, _i32p, _dp]),
    "vg_mono_odom_set_depth": (ctypes.c_int, [_vp, _vp]),
    "vg_mono_odom_warp_image": (ctypes.c_int, [_vp, _vp, _dp, _vp, _vp]),
    "vg_mono_odom_state": (ctypes.c_int, [_vp, _ip]),
    "vg_mono_odom_xi_local": (ctypes.c_int, [_vp, _dp]),
    "vg_mono_odom_xi_global": (ctypes.c_int, [_vp, _dp]),
    "vg_mono_odom_xi_composed": (ctypes.c_int, [_vp, _dp]),
    "vg_mono_odom_num_keyframes": (ctypes.c_int, [_vp, _i64p]),
    "vg_mono_odom_keyframe_increment": (ctypes.c_int, [_vp, ctypes.c_int64, _dp]),
    "vg_mono_odom_get_map": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "vg_mono_odom_map": (ctypes.c_int, [_vp, _vpp, _vpp, _vpp]),
    "vg_mono_odom_integrate": (ctypes.c_int, [_dp, _dp, _dp, _dp]),
    "vg_mono_odom_normalize_scale": (ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "vg_mono_odom_needs_keyframe": (ctypes.c_int, [_vp, _dp, _ip]),
    "vg_mono_odom_camera_motion": (ctypes.c_int, [_dp, _dp, _dp]),
    "vg_mono_odom_compose": (ctypes.c_int, [_dp, _dp, _dp]),
    "vg_mapping_params_default": (None, [_vp]),
    "vg_mapping_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _dp, ctypes.c_int, ctypes.c_int, _vp]),
    "vg_mapping_destroy": (None, [_vp]),
    "vg_mapping_size": (ctypes.c_int, [_vp, _ip, _ip, _ip, _ip]),
    "vg_mapping_feed_odometry": (ctypes.c_int, [_vp, _dp]),
    "vg_mapping_reinit": (ctypes.c_int, [_vp, _dp]),
    "vg_mapping_feed_image": (ctypes.c_int, [_vp, _vp, _i32p, _dp]),
    "vg_mapping_num_frames": (ctypes.c_int, [_vp, _i64p]),
    "vg_mapping_get_frame": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp]),
    "vg_mapping_add_frame": (ctypes.c_int, [_vp, _dp, _vp]),
    "vg_mapping_construct_map": (ctypes.c_int, [_vp, _dp, _vp, _ip]),
    "vg_mapping_select_frame": (ctypes.c_int, [_vp, _dp, ctypes.c_double, _ip]),
    "vg_mapping_alignment": (ctypes.c_int, [_vp, _vp, _vp, _dp, _vp, _vp, _i64p]),
    "vg_mapping_state": (ctypes.c_int, [_vp, _ip]),
    "vg_mapping_map_index": (ctypes.c_int, [_vp, _ip]),
    "vg_mapping_warning": (ctypes.c_int, [_vp, _ip]),
    "vg_mapping_xi_local": (ctypes.c_int, [_vp, _dp]),
    "vg_mapping_xi_inter": (ctypes.c_int, [_vp, _dp]),
    "vg_mapping_xi_composed": (ctypes.c_int, [_vp, _dp]),
    "vg_mapping_get_map": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "vg_mapping_map": (ctypes.c_int, [_vp, _vpp, _vpp, _vpp]),
    "vg_mapping_check_distance": (ctypes.c_int, [_vp, _dp, ctypes.c_double, _ip]),
    "vg_mapping_select_frame_host": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, ctypes.c_double, _ip]),
    "vg_mapping_normalize_scale": (ctypes.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "vg_mapping_relocalized_pose": (ctypes.c_int, [_dp, _dp, _dp]),
    "vg_trajectory_default_options": (None, [_vp]),
    "vg_trajectory_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _ip]),
    "vg_trajectory_destroy": (None, [_vp]),
    "vg_trajectory_size": (ctypes.c_int, [_vp, _ip, _ip, _ip]),
    "vg_trajectory_evaluate": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _dp, _i32p]),
    "vg_trajectory_visual_cov": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _dp, _i32p]),
    "vg_trajectory_gradient": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _dp, _i32p]),
    "vg_trajectory_gradient_points": (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp]),
    "vg_trajectory_poses": (ctypes.c_int, [ctypes.c_int, _ip, _dp, _dp, _dp]),
    "vg_trajectory_optimize": (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp, _dp, _i32p, _i32p]),
    "vg_trajectory_project_board": (ctypes.c_int, [ctypes.c_int, _dp, _vp, _dp, _dp, _i32p]),
    "vg_trajectory_launch_count": (ctypes.c_int, [_vp, _i64p]),
    "vg_dense_ba_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, _dp, _vp, _dp, ctypes.c_int, ctypes.c_int, _vp]),
    "vg_dense_ba_destroy": (None, [_vp]),
    "vg_dense_ba_set_base": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "vg_dense_ba_set_frames": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "vg_dense_ba_pack": (ctypes.c_int, [_vp, _i64p, _vp, _vp, _vp, _vp, _vp]),
    "vg_dense_ba_evaluate": (ctypes.c_int, [_vp, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _dp]),
    "vg_dense_ba_reduce": (ctypes.c_int, [_vp, ctypes.c_double, _dp, _dp]),
    "vg_dense_ba_back_substitute": (ctypes.c_int, [_vp, ctypes.c_double, _dp, _vp, _dp]),
    "vg_dense_ba_solve": (ctypes.c_int, [_vp, _dp, _dp, _vp, _vp, _dp]),
    "vg_hough_params_default": (None, [_vp]),
    "vg_hough_create": (ctypes.c_int, [_vpp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _dp, _dp, _vp]),
    "vg_hough_destroy": (None, [_vp]),
    "vg_hough_size": (ctypes.c_int, [_vp, _ip, _ip]),
    "vg_hough_vote": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _i64p]),
    "vg_hough_detect": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_int, _dp, _i32p, _i32p, _vp]),
    "vg_hough_polynomial": (ctypes.c_int, [_dp, _dp, _dp]),
    "vg_hough_end_points": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _dp, _ip]),
    "vg_hough_trace": (ctypes.c_int, [_dp, _dp, ctypes.c_int, _i32p, _ip]),
    "vg_unproject": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, ctypes.c_int64, _vp, _vp, _vp]),
    "vg_convert_map": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "vg_convert_start": (ctypes.c_int, [ctypes.c_int, _dp, ctypes.c_int, _dp]),
    "vg_convert_fit_default_options": (None, [_vp]),
    "vg_convert_fit": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _vp, _vp]),
    "vg_debug_set": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_longlong]),
    "vg_calib_stream_write": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_double]),
    "vg_calib_stream_copy": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64]),
    "vg_calib_d2h_copies": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, _dp]),
    "vg_calib_fp64_fma": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
}


class StereoParams(ctypes.Structure):
    """struct vg_stereo_params"""
    _fields_ = [(n, ctypes.c_int) for n in ("scale", "u0", "v0", "u_max", "v_max", "x_max", "y_max", "equal_margins",
                                            "num_epipolar_planes", "epipole_margin", "disp_max", "error_max", "verbosity",
                                            "hypotheses", "hypo_difference", "flaw_cost", "desc_length", "desc_resp_thresh",
                                            "n_scales")] + \
               [("scales", ctypes.c_int * 8)] + \
               [(n, ctypes.c_int) for n in ("step_cost", "jump_cost", "image_based_cost", "salient_points_only", "use_uv_cache")]


class MotionStereoParams(ctypes.Structure):
    """struct vg_motion_stereo_params"""
    _fields_ = [("stereo", StereoParams), ("gradient_thresh", ctypes.c_int)]


class MiOptions(ctypes.Structure):
    """struct vg_mi_options; a zero field means the reference's value (MI_DEFAULTS)"""
    _fields_ = [("function_tolerance", ctypes.c_double), ("gradient_tolerance", ctypes.c_double), ("max_iterations", ctypes.c_int)]


class DenseBaOptions(ctypes.Structure):
    """struct vg_dense_ba_options; a zero field means the default (DENSE_BA_DEFAULTS), DENSE_BA_NONE switches off"""
    _fields_ = [("sigma_grey", ctypes.c_double), ("prior_weight", ctypes.c_double), ("grad_thresh", ctypes.c_double),
                ("max_iterations", ctypes.c_int), ("function_tolerance", ctypes.c_double)]


class HoughParams(ctypes.Structure):
    """struct vg_hough_params"""
    _fields_ = [("margin", ctypes.c_int), ("grad_thresh", ctypes.c_double), ("search_size", ctypes.c_int), ("acc_thresh", ctypes.c_double),
                ("acc_delta_thresh", ctypes.c_double), ("horizon_ratio", ctypes.c_double), ("blur_size", ctypes.c_int),
                ("blur_sigma", ctypes.c_double)]


class SparseOdomParams(ctypes.Structure):
    """struct vg_sparse_odom_params"""
    _fields_ = [("max_features", ctypes.c_int), ("match_threshold", ctypes.c_double), ("num_ransac_points", ctypes.c_int),
                ("ransac_iterations", ctypes.c_int), ("inlier_threshold", ctypes.c_double), ("max_lm_iterations", ctypes.c_int),
                ("prior_err_v", ctypes.c_double), ("prior_err_w", ctypes.c_double), ("prior_lambda_t", ctypes.c_double),
                ("prior_lambda_r", ctypes.c_double), ("outlier_gate", ctypes.c_double), ("min_stereo_base", ctypes.c_double)]


class MonoOdomParams(ctypes.Structure):
    """struct vg_mono_odom_params"""
    _fields_ = [(n, ctypes.c_double) for n in ("min_init_dist", "max_dist", "max_angle", "min_scale_length", "max_scale_ratio")] + \
               [("num_scales", ctypes.c_int), ("motion", MotionStereoParams), ("sparse", SparseOdomParams)]


class MappingParams(ctypes.Structure):
    """struct vg_mapping_params; the two new_kf thresholds hold squares"""
    _fields_ = [(n, ctypes.c_double) for n in ("new_kf_distance_thresh", "new_kf_angular_thresh", "min_init_dist", "min_stereo_base",
                                               "dist_thresh")] + [("normalize_scale", ctypes.c_int)] + \
               [(n, ctypes.c_double) for n in ("rotation_tolerance", "min_scale_length", "min_scale_ratio", "max_scale_ratio")] + \
               [("num_scales", ctypes.c_int), ("motion", MotionStereoParams), ("sparse", SparseOdomParams)]


class RenderObject(ctypes.Structure):
    """struct vg_render_object"""
    _fields_ = [("kind", ctypes.c_int), ("texture", ctypes.c_void_p), ("cols", ctypes.c_int), ("rows", ctypes.c_int),
                ("pose", ctypes.c_double * 6), ("width", ctypes.c_double), ("height", ctypes.c_double)]


class TrajectoryQuality(ctypes.Structure):
    """struct vg_trajectory_quality"""
    _fields_ = [("xi_base_cam", ctypes.c_double * 6), ("xi_orig_board", ctypes.c_double * 6), ("turn_radius", ctypes.c_double),
                ("board_cols", ctypes.c_int), ("board_rows", ctypes.c_int), ("board_step", ctypes.c_double),
                ("min_camera_dist", ctypes.c_double), ("min_margin", ctypes.c_double), ("min_cell_size", ctypes.c_double),
                ("prior_variance", ctypes.c_double * 6), ("feature_variance", ctypes.c_double)]


class TrajectoryOptions(ctypes.Structure):
    """struct vg_trajectory_options"""
    _fields_ = [("function_tolerance", ctypes.c_double), ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("max_iterations", ctypes.c_int)]


TRAJECTORY_PARAMS, TRAJECTORY_MAX, TRAJECTORY_MIN_STEPS, TRAJECTORY_MAX_STEPS, TRAJECTORY_MAX_CORNERS = 5, 8, 2, 256, 1024
TRAJECTORY_TERMS, TRAJECTORY_MAX_POINTS = 5, 65535
RENDER_BACKGROUND, RENDER_PLANE, RENDER_MAX_PLANES, RENDER_MIN_SIDE, RENDER_MAX_SIDE, RENDER_COUNTS = 0, 1, 64, 2, 16384, 5
SPARSE_ODOM_REPORT, SPARSE_ODOM_FEED_REPORT = 8, 12
SPARSE_ODOM_OK, SPARSE_ODOM_TOO_FEW_MATCHES, SPARSE_ODOM_NO_HYPOTHESIS = 0, 1, 2
SPARSE_ODOM_FIRST, SPARSE_ODOM_SKIPPED, SPARSE_ODOM_ESTIMATED = 0, 1, 2
MONO_ODOM_BEGIN, MONO_ODOM_SPARSE_INIT, MONO_ODOM_READY = 0, 1, 2
MONO_ODOM_FIRST, MONO_ODOM_WAITING, MONO_ODOM_SPARSE_INIT_KEYFRAME, MONO_ODOM_REFINED, MONO_ODOM_KEYFRAME, MONO_ODOM_DISCARDED = range(6)
MONO_ODOM_REPORT = 16
MAPPING_BEGIN, MAPPING_INIT, MAPPING_LOCALIZE, MAPPING_SLAM = range(4)
MAPPING_WARNING_NONE, MAPPING_WARNING_SCALE, MAPPING_WARNING_ROTATION = range(3)
MAPPING_REPORT = 32
MI_NUM_BINS, MI_VALUE_MAX, MI_ODOMETRY_DAMPING = 8, 255., 0.0002
MI_DEFAULTS = {"function_tolerance": 1e-2, "gradient_tolerance": 1e-3, "max_iterations": 50}
HOUGH_MAX_SIDE, HOUGH_MAX_ACC_SIDE, HOUGH_MAX_SEARCH, HOUGH_MIN_BLUR, HOUGH_MAX_BLUR = 16384, 4096, 8, 3, 15
HOUGH_COUNTS, HOUGH_LINE, HOUGH_MAX_LINES, HOUGH_MAX_TRACE, HOUGH_OK, HOUGH_NO_END_POINTS = 6, 16, 65536, 1500, 0, 1
RECON_QUERY_POINTS, RECON_IMAGE_VALUES, RECON_MINMAX, RECON_ALL_HYPOTHESES = 1, 2, 4, 8
RECON_DEFAULT_VALUES, RECON_SIGMA_VALUE, RECON_QUERY_INDICES, RECON_INDEX_MAPPING = 16, 32, 64, 128
RECON_KNOWN = 1 | 4 | 8 | 16 | 32 | 64 | 128
RECON_MAX_POLYGON = 16


class ReconOutputs(ctypes.Structure):
    """struct vg_recon_outputs"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("indices", "hyp", "points", "sigma_out", "index_map", "item", "valid", "cloud")]
DENSE_BA_MAX_FRAMES, DENSE_BA_TAIL, DENSE_BA_NONE = 8, 5, -1.
DENSE_BA_DEFAULTS = {"sigma_grey": 5., "prior_weight": 1., "grad_thresh": 250., "max_iterations": 150, "function_tolerance": 1e-6}


class ConvertFitOptions(ctypes.Structure):
    """struct vg_convert_fit_options"""
    _fields_ = [("grid_w", ctypes.c_int), ("grid_h", ctypes.c_int), ("max_angle", ctypes.c_double), ("max_iterations", ctypes.c_int),
                ("function_tolerance", ctypes.c_double), ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("use_bounds", ctypes.c_int)]


class ConvertFitSummary(ctypes.Structure):
    """struct vg_convert_fit_summary"""
    _fields_ = [("kept", ctypes.c_int), ("dropped", ctypes.c_int), ("iterations", ctypes.c_int), ("termination", ctypes.c_int),
                ("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double), ("rms", ctypes.c_double),
                ("max_residual", ctypes.c_double)]


CONVERT_MAX_GRID, CONVERT_MAX_SIDE = 1 << 20, 16384


class VisgeomError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("visgeom_amd error %d: %s" % (code, msg))
        self.code = code


_lib = None
_has_hooks = False


def lib_path():
    """the library file this process loads: the default (hooks) build, or -- for the TEST HARNESS only, the library itself
    reads no environment variable -- the file VISGEOM_AMD_LIBRARY names ("production" = lib/production/libvisgeom_amd.so)"""
    sel = os.environ.get("VISGEOM_AMD_LIBRARY")
    if not sel:
        return _build.LIB
    return _build.PRODUCTION_LIB if sel == "production" else sel


class NoDebugHooks(VisgeomError):
    """vg_debug_set on a production library (built without VG_DEBUG_HOOKS: the entry is not exported)"""

    def __init__(self):
        VisgeomError.__init__(self, ERR_STATE, "this library has no debug hooks (production build)")


def has_debug_hooks():
    load()
    return _has_hooks


def load():
    """Load libvisgeom_amd.so.  Raises if it is missing -- build it with
    `python -c "import __graft_entry__ as g; g.build()"`; there is no CPU fallback."""
    global _lib
    global _has_hooks
    if _lib is not None:
        return _lib
    path = lib_path()
    if path != _build.LIB:
        if not os.path.exists(path):
            raise ImportError("VISGEOM_AMD_LIBRARY: %s does not exist (python -m visgeom_amd._build --production)" % path)
    elif not os.path.exists(_build.LIB):
        try:  # build the HIP library in-tree (hipcc cross-compiles); never substitute anything for it
            _build.build()
        except Exception as e:
            raise ImportError("%s is missing and could not be built (%s): run `python -m visgeom_amd._build` "
                              "(needs hipcc). visgeom_amd is HIP-only and has no CPU fallback." % (_build.LIB, e))
    try:  # make torch's bundled HIP runtime the one this process uses (same SONAME, libamdhip64.so.7)
        import torch  # noqa: F401
    except Exception:  # the library also works stand-alone against /opt/rocm
        pass
    L = ctypes.CDLL(path)
    _has_hooks = hasattr(L, "vg_debug_set")
    for name, (res, args) in SIGNATURES.items():
        if name == "vg_debug_set" and not _has_hooks:   # the production library: the one entry it does not export
            continue
        f = getattr(L, name)  # AttributeError here = header / library mismatch
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def check(code):
    if code != OK:
        raise VisgeomError(code, load().vg_last_error().decode("utf-8", "replace"))


def debug_set(name, value):
    """measurement / test hook of the library (vg_debug_set): value 0 restores the default"""
    L = load()
    if not _has_hooks:
        raise NoDebugHooks()
    check(L.vg_debug_set(name.encode(), int(value)))

