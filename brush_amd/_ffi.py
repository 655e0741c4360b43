"""ctypes binding of libbrush_hip.so (include/brush_hip.h).

There is NO fallback path: if the HIP library is missing this module raises, and
every entry point raises on a non-zero status with bh_last_error()'s message.
"""
import ctypes as C
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
# BRUSH_HIP_LIB: developer override used to A/B kernel variants (scripts/ab.sh build); still a HIP build.
LIB_PATH = os.environ.get("BRUSH_HIP_LIB") or os.path.join(_DIR, "libbrush_hip.so")

FLAG_MIP = 1
FLAG_BWD_INFO = 2
FLAG_SMOOTH_CUTOFF = 4
FLAG_SLICED_LISTS = 8

fp = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)


class BhCamera(C.Structure):
    _fields_ = [
        ("vm", C.c_float * 12),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("lim_pos_x", C.c_float), ("lim_pos_y", C.c_float),
        ("lim_neg_x", C.c_float), ("lim_neg_y", C.c_float),
        ("cam_pos", C.c_float * 3),
        ("img_w", C.c_uint32), ("img_h", C.c_uint32),
        ("tile_row_begin", C.c_uint32), ("tile_row_end", C.c_uint32),
        ("model", C.c_uint32), ("dist", C.c_float * 8), ("half_max_render_fov", C.c_float),
    ]


CAMERA_PINHOLE, CAMERA_KANNALA_BRANDT_4, CAMERA_RADIAL_TANGENTIAL_8, CAMERA_THIN_PRISM_FISHEYE = 0, 1, 2, 3


class BhRenderOut(C.Structure):
    _fields_ = [
        ("num_visible", C.c_uint32), ("num_intersections", C.c_uint32),
        ("num_tiles", C.c_uint32), ("tile_bw", C.c_uint32), ("tile_bh", C.c_uint32),
        ("flags", C.c_uint32),
        ("out_img", C.c_void_p), ("out_img_packed", C.c_void_p), ("visible", C.c_void_p),
        ("max_radius", C.c_void_p), ("tile_offsets", C.c_void_p), ("projected", C.c_void_p),
        ("compact_gid_from_isect", C.c_void_p), ("tile_id_from_isect", C.c_void_p),
        ("global_from_compact_gid", C.c_void_p), ("cum_tiles_hit", C.c_void_p),
        ("intersect_counts", C.c_void_p), ("depths_sorted", C.c_void_p),
        ("tile_offsets_far", C.c_void_p), ("list_budget", C.c_uint32), ("num_listed_splats", C.c_uint32),
        ("generation", C.c_uint64),
    ]


class BhHaloOp(C.Structure):
    _fields_ = [("send", C.c_int32), ("peer", C.c_int32), ("row_begin_px", C.c_uint32), ("rows", C.c_uint32)]


class BhLossConfig(C.Structure):
    _fields_ = [("l1_weight", C.c_float), ("ssim_weight", C.c_float), ("bg", C.c_float * 3),
                ("composite_bg", C.c_int32), ("mask", C.c_int32)]


class BhTrainConfig(C.Structure):
    _fields_ = [
        ("lr_mean", C.c_double), ("lr_mean_end", C.c_double), ("total_train_iters", C.c_uint32),
        ("lr_coeffs_dc", C.c_double), ("lr_coeffs_sh_scale", C.c_float), ("lr_opac", C.c_double),
        ("lr_scale", C.c_double), ("lr_rotation", C.c_double), ("ssim_weight", C.c_float),
        ("match_alpha_weight", C.c_float), ("mean_noise_weight", C.c_float), ("background", C.c_float * 3),
        ("median_scene_scale", C.c_float), ("render_mip", C.c_int32), ("exact_lists", C.c_int32), ("growth_stop_iter", C.c_uint32),
    ]


class BhTrainState(C.Structure):
    _fields_ = [
        ("n", C.c_uint32), ("sh_degree", C.c_uint32),
        ("transforms", C.c_void_p), ("sh_coeffs", C.c_void_p), ("raw_opacities", C.c_void_p),
        ("m1_transforms", C.c_void_p), ("m2_transforms", C.c_void_p),
        ("m1_sh", C.c_void_p), ("m2_sh", C.c_void_p),
        ("m1_opac", C.c_void_p), ("m2_opac", C.c_void_p),
        ("refine_weight_norm", C.c_void_p), ("vis_weight", C.c_void_p), ("max_screen_size", C.c_void_p),
        ("step_count", C.c_uint32),
        ("min_scale", C.c_void_p),
    ]


class BhRefineConfig(C.Structure):
    _fields_ = [
        ("iter", C.c_uint32), ("total_train_iters", C.c_uint32), ("growth_stop_iter", C.c_uint32), ("max_splats", C.c_uint32),
        ("growth_grad_threshold", C.c_float), ("growth_select_fraction", C.c_float), ("split_at_screen_size", C.c_float),
        ("opac_decay", C.c_float), ("bounds_center", C.c_float * 3), ("bounds_extent", C.c_float * 3), ("seed", C.c_uint64),
    ]


class BhRefineStats(C.Structure):
    _fields_ = [("num_added", C.c_uint32), ("num_split_oversized", C.c_uint32), ("num_split_high_grad", C.c_uint32),
                ("num_pruned", C.c_uint32), ("num_pruned_non_finite", C.c_uint32), ("total_splats", C.c_uint32),
                ("num_resampled", C.c_uint32)]


class BhTrainBatch(C.Structure):
    _fields_ = [
        ("camera", BhCamera), ("gt_packed", C.c_void_p), ("has_alpha", C.c_int32), ("alpha_is_mask", C.c_int32),
        ("background", C.c_float * 3), ("noise_samples", C.c_void_p), ("device_noise", C.c_int32), ("noise_seed", C.c_uint64),
        ("image_hook", C.c_void_p), ("image_hook_user", C.c_void_p), ("exchange_mode", C.c_int32), ("strip_loss", C.c_int32),
        ("view_id", C.c_uint32),
    ]


class BhTrainStats(C.Structure):
    _fields_ = [("num_visible", C.c_uint32), ("num_intersections", C.c_uint32), ("lr_mean", C.c_double), ("loss", C.c_float),
                ("exchange_rows", C.c_uint32)]


class BhPlyInfo(C.Structure):
    _fields_ = [("num_splats", C.c_uint64), ("sh_degree", C.c_uint32), ("row_floats", C.c_uint32), ("body_offset", C.c_uint64),
                ("render_mode", C.c_int32), ("has_up_axis", C.c_int32), ("up_axis", C.c_float * 3), ("compressed", C.c_int32)]


GRAD_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)
IMAGE_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)

# every symbol include/brush_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "bh_create": (C.c_void_p, [C.c_int, C.c_void_p, C.c_int]),
    "bh_destroy": (None, [C.c_void_p]),
    "bh_last_error": (C.c_char_p, [C.c_void_p]),
    "bh_sync": (C.c_int, [C.c_void_p]),
    "bh_version": (C.c_char_p, []),
    "bh_abi_version": (C.c_uint32, []),
    "bh_struct_size": (C.c_uint32, [C.c_uint32]),
    "bh_last_list_counts": (C.c_int, [C.c_void_p, u32p, u32p]),
    "bh_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "bh_option_count": (C.c_int, []),
    "bh_option_name": (C.c_char_p, [C.c_int]),
    "bh_option_help": (C.c_char_p, [C.c_int]),
    "bh_camera_setup": (C.c_int, [fp, fp, C.c_double, C.c_double, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(BhCamera)]),
    "bh_camera_setup_model": (C.c_int, [fp, fp, C.c_double, C.c_double, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, fp, C.POINTER(BhCamera)]),
    "bh_fov_to_focal": (C.c_double, [C.c_double, C.c_uint32, C.c_uint32, fp]),
    "bh_focal_to_fov": (C.c_double, [C.c_double, C.c_uint32, C.c_uint32, fp]),
    "bh_render_forward": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, fp, C.c_uint32, C.POINTER(BhRenderOut)]),
    "bh_set_list_slicing": (C.c_int, [C.c_void_p, C.c_float]),
    "bh_set_view_id": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bh_set_list_cut_threshold": (C.c_int, [C.c_void_p, C.c_uint32]),
    "bh_last_list_share": (C.c_float, [C.c_void_p]),
    "bh_far_slices_queued": (C.c_uint32, [C.c_void_p]),
    "bh_view_table_count": (C.c_uint32, [C.c_void_p]),
    "bh_render_backward": (C.c_int, [C.c_void_p] * 9),
    "bh_render_backward_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut)] + [C.c_void_p] * 8),
    "bh_render_retain": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut)]),
    "bh_render_release": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut)]),
    "bh_last_v_combined": (C.c_void_p, [C.c_void_p]),
    "bh_last_render_out": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut)]),
    "bh_radix_argsort": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bh_tile_sort_offsets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bh_prefix_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bh_image_loss_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BhLossConfig), C.c_void_p]),
    "bh_image_loss_value_and_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BhLossConfig), C.c_float, C.c_void_p, C.c_void_p]),
    "bh_image_loss_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BhLossConfig), C.c_void_p]),
    "bh_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_float, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_float]),
    "bh_gather_stats": (C.c_int, [C.c_void_p] * 7 + [C.c_uint64]),
    "bh_refine_plan": (C.c_int, [C.c_void_p, C.POINTER(BhRefineConfig), C.POINTER(BhTrainState), C.POINTER(BhRefineStats)]),
    "bh_refine_plan_flags": (C.c_void_p, [C.c_void_p, C.c_int]),
    "bh_refine_apply": (C.c_int, [C.c_void_p, C.POINTER(BhRefineConfig), C.POINTER(BhTrainState), C.POINTER(BhTrainState)]),
    "bh_splat_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "bh_knn_log_scales": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "bh_fold_min_scale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bh_fold_min_scale_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bh_compute_min_scale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, fp, C.c_uint32, C.c_float, C.c_void_p]),
    "bh_pup_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bh_pup_accumulate_view": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "bh_pup_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bh_eval_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "bh_eval_view": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 3),
    "bh_decimate_to_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 9),
    "bh_splat_to_ply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, fp, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bh_ply_parse_header": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(BhPlyInfo)]),
    "bh_ply_vertex_has_property": (C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p]),
    "bh_splats_from_ply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bh_splats_from_ply_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bh_uploader_create": (C.c_void_p, [C.c_void_p, C.c_uint64, C.c_uint32]),
    "bh_uploader_destroy": (None, [C.c_void_p]),
    "bh_uploader_last_error": (C.c_char_p, [C.c_void_p]),
    "bh_uploader_begin": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "bh_uploader_commit": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    "bh_uploader_submit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    "bh_uploader_acquire": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "bh_uploader_release": (C.c_int, [C.c_void_p, C.c_int]),
    "bh_comm_unique_id": (C.c_int, [C.c_void_p]),
    "bh_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "bh_comm_destroy": (C.c_int, [C.c_void_p]),
    "bh_comm_world": (C.c_int, [C.c_void_p]),
    "bh_allreduce_sum_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "bh_allreduce_max_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "bh_allgather_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "bh_forget_views": (C.c_int, [C.c_void_p]),
    "bh_comm_rank": (C.c_int, [C.c_void_p]),
    "bh_comm_selftest": (C.c_int, [C.c_void_p]),
    "bh_strip_halo_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "bh_exchange_strip_halos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "bh_train_step": (C.c_int, [C.c_void_p, C.POINTER(BhTrainConfig), C.POINTER(BhTrainState), C.POINTER(BhTrainBatch), C.c_void_p, C.c_void_p, C.c_float, C.POINTER(BhTrainStats)]),
    "bh_sample_background": (None, [C.c_uint64, C.c_uint32, fp, C.c_float, fp]),
    "bh_normal_samples": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]),
    "bh_philox4x32_10": (None, [u32p, u32p, u32p]),
    "bh_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "bh_profile_fetch": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), fp, u32p, C.c_int]),
}

# every symbol include/brush_hip_lpips.h declares (LPIPS, a header of its own on top of brush_hip.h), bound on the same handle
LPIPS_PARAM_COUNT = 14716160   # BH_LPIPS_PARAM_COUNT
LPIPS_SYMBOLS = {
    "bh_lpips_create": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_float), C.c_uint64]),
    "bh_lpips_destroy": (None, [C.c_void_p]),
    "bh_lpips_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_void_p]),
    "bh_lpips_value_and_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_float,
                                          C.c_void_p, C.c_void_p]),
    "bh_train_set_lpips": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float]),
}

# every symbol include/brush_hip_compressed_ply.h declares (compressed PLY export, a header of its own on top of brush_hip.h)
COMPRESSED_PLY_SYMBOLS = {
    "bh_splat_to_compressed_ply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, fp,
                                             C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
}

# every symbol include/brush_hip_image.h declares (mask merge + resampling of LoadImage::load, a header of its own on top of brush_hip.h)
FILTER_LANCZOS3, FILTER_TRIANGLE = 0, 1   # BH_FILTER_*


class BhViewLoad(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("channels", C.c_uint32), ("mask_w", C.c_uint32), ("mask_h", C.c_uint32),
                ("invert_mask", C.c_int32), ("mask_offset", C.c_uint64), ("max_resolution", C.c_uint32), ("scale", C.c_float),
                ("premultiply", C.c_int32), ("reserved", C.c_uint32)]


IMAGE_SYMBOLS = {
    "bh_view_output_size": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, u32p, u32p]),
    "bh_resize_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "bh_uploader_commit_view": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BhViewLoad)]),
}

# every symbol include/brush_hip_depth.h declares (depth maps of a saved forward and their gradient, a header of its own on top of brush_hip.h)
DEPTH_ACCUMULATED, DEPTH_EXPECTED, DEPTH_MEDIAN = 0, 1, 2   # BH_DEPTH_*
DEPTH_SYMBOLS = {
    "bh_render_depth": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_uint32, C.c_void_p]),
    "bh_render_backward_depth_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7),
}

# every symbol include/brush_hip_pose.h declares (the pose gradient of a saved forward and the host arithmetic of a pose update)
dp = C.POINTER(C.c_double)
POSE_SYMBOLS = {
    "bh_render_backward_pose_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut)] + [C.c_void_p] * 9),
    "bh_train_set_pose_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bh_pose_twist": (C.c_int, [fp, fp, dp]),
    "bh_camera_apply_twist": (C.c_int, [C.POINTER(BhCamera), dp]),
}

# every symbol include/brush_hip_exposure.h declares (per-view exposure compensation: a device table of affine colour transforms)
EXPOSURE_SYMBOLS = {
    "bh_exposure_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "bh_exposure_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bh_exposure_set_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, fp]),
    "bh_exposure_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, fp]),
    "bh_exposure_get_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, fp]),
    "bh_exposure_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, dp, dp, u32p]),
    "bh_exposure_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, dp, dp, C.c_uint32]),
    "bh_exposure_set_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bh_exposure_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bh_exposure_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "bh_train_set_exposure": (C.c_int, [C.c_void_p, C.c_void_p]),
}

# every symbol include/brush_hip_bilagrid.h declares (per-view bilateral grids: a device table of grids of affine colour transforms)
BILAGRID_SYMBOLS = {
    "bh_bilagrid_create": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "bh_bilagrid_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bh_bilagrid_dims": (C.c_int, [C.c_void_p, C.c_void_p, u32p, u32p, u32p, u32p]),
    "bh_bilagrid_set_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, fp]),
    "bh_bilagrid_get_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, fp]),
    "bh_bilagrid_get_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, fp]),
    "bh_bilagrid_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, fp, fp, u32p]),
    "bh_bilagrid_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, fp, fp, C.c_uint32]),
    "bh_bilagrid_set_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bh_bilagrid_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bh_bilagrid_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_int]),
    "bh_bilagrid_tv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "bh_train_set_bilagrid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float]),
}

# every symbol include/brush_hip_depth_loss.h declares (depth supervision: the fused depth loss, the step's depth term, depth metrics)
DEPTH_LOSS_L1, DEPTH_LOSS_DISPARITY = 0, 1   # BH_DEPTH_LOSS_*


class BhDepthTarget(C.Structure):
    _fields_ = [("gt", C.c_void_p), ("h", C.c_uint32), ("w", C.c_uint32), ("kind", C.c_uint32), ("weight", C.c_float),
                ("scale", C.c_float), ("offset", C.c_float)]


DEPTH_LOSS_SYMBOLS = {
    "bh_depth_loss_value_and_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BhDepthTarget), C.c_void_p, C.c_void_p]),
    "bh_train_set_depth": (C.c_int, [C.c_void_p, C.POINTER(BhDepthTarget)]),
    "bh_eval_depth_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BhDepthTarget), C.c_void_p]),
}

# every symbol include/brush_hip_normal.h declares (normal maps of a saved forward, normals from a depth map, and their gradients)
NORMAL_ACCUMULATED, NORMAL_UNIT = 0, 1   # BH_NORMAL_*
NORMAL_SYMBOLS = {
    "bh_splat_normals": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_void_p, C.c_uint64, C.c_void_p]),
    "bh_render_normal": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_uint32, C.c_void_p]),
    "bh_render_backward_normal_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
                                        + [C.c_void_p] * 7),
    "bh_depth_to_normal": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bh_depth_to_normal_backward": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
}

# every symbol include/brush_hip_normal_loss.h declares (normal consistency: the fused operator and the step's normal term)
class BhNormalTermConfig(C.Structure):
    _fields_ = [("weight", C.c_float), ("reserved", C.c_uint32 * 3)]


NORMAL_LOSS_SYMBOLS = {
    "bh_normal_consistency_value_and_grad": (C.c_int, [C.c_void_p, C.POINTER(BhCamera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                       C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bh_train_set_normal": (C.c_int, [C.c_void_p, C.POINTER(BhNormalTermConfig)]),
}

# every symbol include/brush_hip_distortion.h declares (distortion maps, their backward, the loss and the step's distortion term)
DISTORTION_Z, DISTORTION_NDC = 0, 1


class BhDistortionConfig(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("near_z", C.c_float), ("far_z", C.c_float), ("reserved", C.c_uint32)]


class BhDistortionTermConfig(C.Structure):
    _fields_ = [("weight", C.c_float), ("kind", C.c_uint32), ("near_z", C.c_float), ("far_z", C.c_float)]


DISTORTION_SYMBOLS = {
    "bh_render_distortion": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.POINTER(BhDistortionConfig), C.c_void_p]),
    "bh_render_distortion_moments": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.POINTER(BhDistortionConfig), C.c_void_p]),
    "bh_render_backward_distortion_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                      C.c_void_p, C.POINTER(BhDistortionConfig)] + [C.c_void_p] * 7),
    "bh_distortion_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]),
    "bh_train_set_distortion": (C.c_int, [C.c_void_p, C.POINTER(BhDistortionTermConfig)]),
}

# every symbol include/brush_hip_mesh.h declares (mesh extraction: TSDF fusion of depth maps, marching tetrahedra, the mesh PLY)
TSDF_MAX_BATCH = 8   # BH_TSDF_MAX_BATCH


class BhTsdfGrid(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32),
                ("trunc", C.c_float), ("max_weight", C.c_float), ("reserved", C.c_uint32), ("tw", C.c_void_p), ("rgb", C.c_void_p)]


class BhTsdfIntegrateConfig(C.Structure):
    _fields_ = [("depth_min", C.c_float), ("depth_max", C.c_float), ("alpha_min", C.c_float), ("reserved", C.c_uint32)]


MESH_SYMBOLS = {
    "bh_tsdf_clear": (C.c_int, [C.c_void_p, C.POINTER(BhTsdfGrid)]),
    "bh_tsdf_integrate": (C.c_int, [C.c_void_p, C.POINTER(BhTsdfGrid), C.c_uint32, C.POINTER(BhCamera), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.POINTER(BhTsdfIntegrateConfig)]),
    "bh_tsdf_extract_count": (C.c_int, [C.c_void_p, C.POINTER(BhTsdfGrid), u32p, u32p]),
    "bh_tsdf_extract": (C.c_int, [C.c_void_p, C.POINTER(BhTsdfGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, u32p, u32p]),
    "bh_mesh_to_ply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
}

# every symbol include/brush_hip_sparse_mesh.h declares (sparse TSDF volumes: block-allocated fusion and mesh extraction)
SPTSDF_BLOCK = 8        # BH_SPTSDF_BLOCK
SPTSDF_MAX_DIM = 8192   # BH_SPTSDF_MAX_DIM
SPTSDF_MAX_STEPS = 64   # BH_SPTSDF_MAX_STEPS


class BhSparseTsdf(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_size", C.c_float), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32),
                ("trunc", C.c_float), ("max_weight", C.c_float), ("n_blocks", C.c_uint32), ("bits", C.c_void_p), ("rank", C.c_void_p),
                ("keys", C.c_void_p), ("tw", C.c_void_p), ("rgb", C.c_void_p)]


_sptsdf_views = [C.c_void_p, C.POINTER(BhSparseTsdf), C.c_uint32, C.POINTER(BhCamera), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(BhTsdfIntegrateConfig)]
SPARSE_MESH_SYMBOLS = {
    "bh_sptsdf_mark_clear": (C.c_int, [C.c_void_p, C.POINTER(BhSparseTsdf)]),
    "bh_sptsdf_mark": (C.c_int, _sptsdf_views),
    "bh_sptsdf_commit": (C.c_int, [C.c_void_p, C.POINTER(BhSparseTsdf), C.c_uint32, u32p]),
    "bh_sptsdf_clear": (C.c_int, [C.c_void_p, C.POINTER(BhSparseTsdf)]),
    "bh_sptsdf_integrate": (C.c_int, _sptsdf_views),
    "bh_sptsdf_extract_count": (C.c_int, [C.c_void_p, C.POINTER(BhSparseTsdf), u32p, u32p]),
    "bh_sptsdf_extract": (C.c_int, [C.c_void_p, C.POINTER(BhSparseTsdf), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, u32p, u32p]),
    "bh_sptsdf_to_dense": (C.c_int, [C.c_void_p, C.POINTER(BhSparseTsdf), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(BhTsdfGrid)]),
}

# every symbol include/brush_hip_features.h declares (feature maps: N-channel splat features, their backward and the fused losses)
FEATURE_MAX_CHANNELS = 256   # BH_FEATURE_MAX_CHANNELS
FEATURE_LOSS_L1, FEATURE_LOSS_CROSS_ENTROPY = 0, 1   # BH_FEATURE_LOSS_*


class BhFeatureTarget(C.Structure):
    _fields_ = [("target", C.c_void_p), ("h", C.c_uint32), ("w", C.c_uint32), ("channels", C.c_uint32), ("kind", C.c_uint32),
                ("weight", C.c_float), ("reserved", C.c_uint32)]


FEATURE_SYMBOLS = {
    "bh_render_features": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_uint32, C.c_void_p]),
    "bh_render_backward_features_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 9),
    "bh_feature_loss_value_and_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BhFeatureTarget), C.c_void_p, C.c_void_p]),
}

# every symbol include/brush_hip_feature_train.h declares (feature fields trained with the splats: the step's feature term and the row
# carry through a refine)
CARRY_COPY, CARRY_ZERO_SPLIT = 0, 1   # BH_CARRY_*
CARRY_MAX_CHANNELS = 4096             # BH_CARRY_MAX_CHANNELS


class BhFeatureField(C.Structure):
    _fields_ = [("features", C.c_void_p), ("m1", C.c_void_p), ("m2", C.c_void_p), ("n", C.c_uint32), ("channels", C.c_uint32),
                ("step", C.c_uint32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("reserved", C.c_uint32)]


FEATURE_TRAIN_SYMBOLS = {
    "bh_train_set_features": (C.c_int, [C.c_void_p, C.POINTER(BhFeatureField), C.POINTER(BhFeatureTarget)]),
    "bh_refine_carry_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
}

# every symbol include/brush_hip_scene.h declares (scene editing: a similarity transform of the splats with their SH rotation, the same
# transform of a camera, a region select)
REGION_BOX, REGION_ELLIPSOID = 0, 1   # BH_REGION_*


class BhSceneTransform(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("rot", C.c_float * 9), ("quat", C.c_float * 4),
                ("trans", C.c_float * 3), ("scale", C.c_float), ("log_scale", C.c_float), ("sh_rot", C.c_float * 164),
                ("reserved", C.c_uint32 * 2)]


class BhSceneRegion(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("invert", C.c_uint32), ("center", C.c_float * 3), ("half_extent", C.c_float * 3),
                ("rot", C.c_float * 9), ("min_raw_opacity", C.c_float), ("reserved", C.c_uint32)]


SCENE_SYMBOLS = {
    "bh_scene_transform_make": (C.c_int, [dp, dp, C.c_double, C.POINTER(BhSceneTransform)]),
    "bh_scene_transform_compose": (C.c_int, [C.POINTER(BhSceneTransform), C.POINTER(BhSceneTransform), C.POINTER(BhSceneTransform)]),
    "bh_scene_transform_invert": (C.c_int, [C.POINTER(BhSceneTransform), C.POINTER(BhSceneTransform)]),
    "bh_camera_apply_scene_transform": (C.c_int, [C.POINTER(BhCamera), C.POINTER(BhSceneTransform), C.POINTER(BhCamera)]),
    "bh_splats_transform": (C.c_int, [C.c_void_p, C.POINTER(BhSceneTransform), C.c_uint32, C.c_uint32] + [C.c_void_p] * 6),
    "bh_splats_select_region": (C.c_int, [C.c_void_p, C.POINTER(BhSceneRegion), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, u32p]),
}

# every symbol include/brush_hip_lift.h declares (mask lifting: per-splat blend-weight votes from 2-D label maps, assign, select)
LIFT_MAX_LABELS, LIFT_UNASSIGNED, LIFT_ANY_LABEL = 256, 255, 0xFFFFFFFF   # BH_LIFT_*
LIFT_VOTE_ONE = 16777216.0   # a weight of 1 in raw units (2^24)


class BhLiftSelect(C.Structure):
    _fields_ = [("label", C.c_uint32), ("min_share", C.c_float), ("min_weight", C.c_float), ("min_max_weight", C.c_float),
                ("min_pixels", C.c_uint32), ("invert", C.c_uint32)]


LIFT_SYMBOLS = {
    "bh_lift_accumulate": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bh_lift_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]),
    "bh_lift_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BhLiftSelect), C.c_void_p]),
}

# every symbol include/brush_hip_envmap.h declares (environment maps: a learned cubemap behind the splats, trained in the step)
ENVMAP_MAX_RESOLUTION = 1024   # BH_ENVMAP_MAX_RESOLUTION
ENVMAP_SYMBOLS = {
    "bh_envmap_create": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "bh_envmap_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bh_envmap_set_params": (C.c_int, [C.c_void_p, C.c_void_p, fp]),
    "bh_envmap_get_params": (C.c_int, [C.c_void_p, C.c_void_p, fp]),
    "bh_envmap_get_grad": (C.c_int, [C.c_void_p, C.c_void_p, fp]),
    "bh_envmap_get_state": (C.c_int, [C.c_void_p, C.c_void_p, fp, fp, u32p]),
    "bh_envmap_set_state": (C.c_int, [C.c_void_p, C.c_void_p, fp, fp, C.c_uint32]),
    "bh_envmap_set_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bh_envmap_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BhCamera), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "bh_envmap_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(BhCamera), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]),
    "bh_train_set_envmap": (C.c_int, [C.c_void_p, C.c_void_p]),
}

# every symbol include/brush_hip_intrinsics.h declares (the intrinsics gradient of a saved forward, the step's attachment, the host update)
class BhCameraGradTerms(C.Structure):
    _fields_ = [("v_depth", C.c_void_p), ("v_normal", C.c_void_p), ("v_distortion", C.c_void_p), ("depth_mode", C.c_uint32),
                ("normal_mode", C.c_uint32), ("distortion", BhDistortionConfig)]


INTRINSICS_SYMBOLS = {
    "bh_render_backward_intrinsics_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut)] + [C.c_void_p] * 10),
    "bh_render_backward_camera_saved": (C.c_int, [C.c_void_p, C.POINTER(BhRenderOut), C.c_void_p, C.POINTER(BhCameraGradTerms)] + [C.c_void_p] * 9),
    "bh_train_set_intrinsics_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bh_camera_set_intrinsics": (C.c_int, [C.POINTER(BhCamera), C.c_double, C.c_double, C.c_double, C.c_double]),
}

ABI_VERSION = 7   # the BH_ABI_VERSION of include/brush_hip.h these mirrors were written against
# bh_struct_size index -> mirror (the BH_STRUCT_* order of the header)
STRUCT_MIRRORS = (BhCamera, BhRenderOut, BhLossConfig, BhTrainConfig, BhTrainState, BhTrainBatch, BhTrainStats, BhRefineConfig, BhRefineStats, BhPlyInfo)

_lib = None
_lib_th = None
# the test suite's fault-injection build (csrc/Makefile, -DBH_TEST_HOOKS): never loaded by product code
TEST_HOOKS_LIB_PATH = os.path.join(_DIR, "libbrush_hip_testhooks.so")
TEST_HOOK_SYMBOLS = {"bh_debug_fill_train_scratch": (C.c_int, [C.c_void_p, C.c_uint32]),
                     "bh_debug_split_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
                     # (ctx, keys, minmax, counts, n, out_keys, out_vals, cum, spl, spl_written, totals_out[512]): api.hip
                     "bh_debug_depth_sort": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
                     # (ctx, keys, minmax, counts, n, out_keys, out_vals, cum, spl, cap, stride, ctr_out[256], fell_back): api.hip
                     "bh_debug_depth_deal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
                     "bh_debug_dsort_deal_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
                     "bh_debug_set_deal_capacity": (C.c_int, [C.c_void_p, C.c_uint32]),
                     # (ctx, img_hwc4, gt_packed, h, w, cfg, alpha_weight, tile_y0, tile_y1, loss_out, v_output): api.hip
                     "bh_debug_image_loss_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(BhLossConfig), C.c_float, C.c_uint32,
                                                              C.c_uint32, C.c_void_p, C.c_void_p])}


class BrushHipError(RuntimeError):
    pass


def _bind(path, symbols):
    if not os.path.exists(path):
        raise BrushHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    lib = C.CDLL(path)
    for name, (res, args) in symbols.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    # ABI guard: the library fills these structs with ITS layout; a mirror of another revision would be overrun
    if lib.bh_abi_version() != ABI_VERSION:
        raise BrushHipError("%s speaks ABI %d, this binding ABI %d" % (path, lib.bh_abi_version(), ABI_VERSION))
    for i, mirror in enumerate(STRUCT_MIRRORS):
        if lib.bh_struct_size(i) != C.sizeof(mirror):
            raise BrushHipError("%s: sizeof(%s) is %d in the library, %d in this binding" % (path, mirror.__name__, lib.bh_struct_size(i), C.sizeof(mirror)))
    return lib


def load():
    """Load libbrush_hip.so and bind every declared symbol. Raises if the library is absent."""
    global _lib
    if _lib is None:
        _lib = _bind(LIB_PATH, dict(SYMBOLS, **LPIPS_SYMBOLS, **COMPRESSED_PLY_SYMBOLS, **IMAGE_SYMBOLS, **DEPTH_SYMBOLS, **POSE_SYMBOLS, **EXPOSURE_SYMBOLS, **BILAGRID_SYMBOLS, **DEPTH_LOSS_SYMBOLS, **NORMAL_SYMBOLS, **NORMAL_LOSS_SYMBOLS, **DISTORTION_SYMBOLS, **MESH_SYMBOLS, **SPARSE_MESH_SYMBOLS, **FEATURE_SYMBOLS, **FEATURE_TRAIN_SYMBOLS, **SCENE_SYMBOLS, **LIFT_SYMBOLS, **ENVMAP_SYMBOLS, **INTRINSICS_SYMBOLS))
    return _lib


def load_test_hooks():
    """TESTS ONLY: the fault-injection build of the same sources (a second, independent copy of the library in the process);
    pass it to Context(lib=...)."""
    global _lib_th
    if _lib_th is None:
        _lib_th = _bind(TEST_HOOKS_LIB_PATH, dict(SYMBOLS, **LPIPS_SYMBOLS, **COMPRESSED_PLY_SYMBOLS, **IMAGE_SYMBOLS, **DEPTH_SYMBOLS, **POSE_SYMBOLS, **EXPOSURE_SYMBOLS, **BILAGRID_SYMBOLS, **DEPTH_LOSS_SYMBOLS, **NORMAL_SYMBOLS, **NORMAL_LOSS_SYMBOLS, **DISTORTION_SYMBOLS, **MESH_SYMBOLS, **SPARSE_MESH_SYMBOLS, **FEATURE_SYMBOLS, **FEATURE_TRAIN_SYMBOLS, **SCENE_SYMBOLS, **LIFT_SYMBOLS, **ENVMAP_SYMBOLS, **INTRINSICS_SYMBOLS,
                                                   **TEST_HOOK_SYMBOLS))
    return _lib_th
