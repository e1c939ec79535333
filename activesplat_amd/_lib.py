"""ctypes binding of the C ABI in include/gsplat_hip.h (libgsplat_hip.so, hipcc-built for gfx950).

There is no CPU fallback: `get()` raises if the HIP library is missing.  `load_for_tests(path)` exists
only so that tests/ can point the same binding at the host-emulated build of the kernel sources
(tests/hipemu) while debugging kernel logic without a GPU; the product never calls it.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsplat_hip.so")

_lib = None
_emulated = False


class GsCamera(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("sh_degree", C.c_int32),
                ("sh_coeffs", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("scale_modifier", C.c_float), ("num_views", C.c_int32), ("bg", C.c_void_p),
                ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p)]


class GsGeomLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_bytes", "geom", "rect", "tiles_touched", "offsets", "block_sums", "clamped",
                                          "tile_total", "tile_base", "sh_jac", "depth_bits")]


class GsImageLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_bytes", "ranges", "final_T", "n_contrib", "split_state")]


class GsAdamTensor(C.Structure):
    _fields_ = [("n", C.c_int64), ("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("step", C.c_int32),
                ("reserved", C.c_int32)]


class GsRowTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("grad", C.c_void_p),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("width", C.c_int32),
                ("step", C.c_int32)]


class GsBinLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_bytes", "path", "pairs", "keys_unsorted", "vals_unsorted", "keys_sorted",
                                          "sort_temp", "segments", "seg_T", "pairs_alt")]


class GsDbscanLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_bytes", "mask_bits", "core_bits", "root_bits", "word_prefix", "parent", "root", "row_range")]


class GsEvalLayout(C.Structure):
    _fields_ = [("total_bytes", C.c_uint64), ("ms_ssim_defined", C.c_int32), ("levels", C.c_int32), ("level_width", C.c_int32 * 5),
                ("level_height", C.c_int32 * 5)]


class GsHullLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_bytes", "cluster_status")]


class GsMeshLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_bytes", "total", "records", "rects", "tile_count", "tile_offset", "list")]


TEXTURE_MAX_LEVELS = 15
WRAP_REPEAT, WRAP_CLAMP, WRAP_MIRROR = 0, 1, 2


class GsTextureDesc(C.Structure):
    """one texture of the mesh sensor's pool (include/gsplat_hip.h); levels and level_offset are gs_texture_layout's"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "wrap_s", "wrap_t", "levels", "reserved")] + [("level_offset", C.c_uint64 * TEXTURE_MAX_LEVELS)]


class GsImageGrads(C.Structure):
    """dL/d of the four image outputs (include/gsplat_hip.h); all but dL_dcolor nullable"""
    _fields_ = [(n, C.c_void_p) for n in ("dL_dcolor", "dL_ddepth", "dL_dopacity", "dL_ddepth_sq")]


SORT_AUTO, SORT_TILE_LDS, SORT_RADIX = 0, 1, 2


#: the GS_ABI_VERSION of include/gsplat_hip.h this binding was written against (checked when a library is bound)
ABI_VERSION = 28

vp, i32, u32, i64, u64, f32, f64, cint = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_int

# every symbol include/gsplat_hip.h declares -> (restype, argtypes), in the header's order, each under its parameter names (tests check the library
# exports all of them and that return type, parameter count and every parameter's class agree with the header's prototype)
BINDINGS = {
    # (P, view_width, num_views, virtual_P, atlas_width, view_stride)
    "gs_atlas_layout": (cint, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    # (P, width, height, out)
    "gs_geom_layout": (cint, [i32, i32, i32, C.POINTER(GsGeomLayout)]),
    # (width, height, out)
    "gs_image_layout": (cint, [i32, i32, C.POINTER(GsImageLayout)]),
    # (D, max_tile_instances, width, height, out)
    "gs_bin_layout": (cint, [i64, u32, i32, i32, C.POINTER(GsBinLayout)]),
    # (path)
    "gs_set_sort_path": (cint, [i32]),
    # (on)
    "gs_set_forward_segments": (cint, [i32]),
    # (max_tiles)
    "gs_set_half_quadrants": (cint, [i32]),
    # (pieces, min_tiles)
    "gs_set_backward_chain": (cint, [i32, i32]),
    # (on)
    "gs_set_backward_chain_tickets": (cint, [i32]),
    # (polls)
    "gs_set_backward_chain_polls": (cint, [i32]),
    # (mode, param)
    "gs_set_forward_priority": (cint, [i32, f32]),
    # (host_word)
    "gs_async_status_word": (cint, [C.POINTER(C.POINTER(u32))]),
    # ()
    "gs_async_status_clear": (cint, []),
    # (target, nearest, level)
    "gs_recorded_cut": (cint, [u32, C.POINTER(u32), C.POINTER(i32)]),
    # (segments)
    "gs_set_backward_segments": (cint, [i32]),
    # (P)
    "gs_backward_scratch_bytes": (u64, [i32]),
    # ()
    "gs_last_error": (C.c_char_p, []),
    # ()
    "gs_version": (C.c_char_p, []),
    # ()
    "gs_abi_version": (i32, []),
    # (on)
    "gs_profile_enable": (cint, [i32]),
    # ()
    "gs_profile_stage_count": (i32, []),
    # (stage)
    "gs_profile_stage_name": (C.c_char_p, [i32]),
    # (ms_sum, calls, n_stages)
    "gs_profile_collect": (cint, [vp, vp, i32]),
    # (cam, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii, geom_state, image_state, d_counts, h_counts, want_backward, stream)
    "gs_preprocess_forward": (cint, [C.POINTER(GsCamera), i32] + [vp] * 12 + [i32, vp]),
    # (cam, P, D, max_tile_instances, geom_state, bin_state, point_list, image_state, out_color, out_depth, out_opacity, out_depth_sq, backward_scratch, stream)
    "gs_render_forward": (cint, [C.POINTER(GsCamera), i32, i64, u32] + [vp] * 10),
    # (cam, P, D, means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, radii, geom_state, point_list, image_state, dL_dcolor, dL_ddepth, dL_dmeans2D, dL_dmeans3D, dL_dopacities, dL_dcolors_precomp, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D, scratch, scratch_zeroed, have_sh_jacobian, stream)
    "gs_render_backward": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 21 + [i32, i32, vp]),
    # (cam, P, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, max_2D_radius, seen, radii, geom_state, image_state, d_counts, h_counts, want_backward, stream)
    "gs_preprocess_forward_raw": (cint, [C.POINTER(GsCamera), i32] + [vp] * 7 + [i32] + [vp] * 7 + [i32, vp]),
    # (cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, accumulate, radii, geom_state, point_list, image_state, dL_dcolor, dL_ddepth, dL_dmeans2D, dL_dmeans3D, dL_dlogit_opacities, dL_dcolors_precomp, dL_dshs, dL_dlog_scales, dL_dunnorm_rotations, scratch, scratch_zeroed, have_sh_jacobian, stream)
    "gs_render_backward_raw": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 7 + [i32, i32] + [vp] * 14 + [i32, i32, vp]),
    # (P)
    "gs_pose_grad_scratch_bytes": (u64, [i32]),
    # (cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, accumulate, radii, geom_state, point_list, image_state, dL_dcolor, dL_ddepth, dL_dmeans2D, dL_dmeans3D, dL_dlogit_opacities, dL_dcolors_precomp, dL_dshs, dL_dlog_scales, dL_dunnorm_rotations, scratch, scratch_zeroed, have_sh_jacobian, pose_only, dL_dpose7, pose_scratch, stream)
    "gs_render_backward_raw_pose": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 7 + [i32, i32] + [vp] * 14 + [i32, i32, i32, vp, vp, vp]),
    # (cam, P, D, means3D, shs, colors_precomp, scales, rotations, cov3D_precomp, radii, geom_state, point_list, image_state, grads, dL_dmeans2D, dL_dmeans3D, dL_dopacities, dL_dcolors_precomp, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D, scratch, scratch_zeroed, have_sh_jacobian, stream)
    "gs_render_backward_grads": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 10 + [C.POINTER(GsImageGrads)] + [vp] * 9 + [i32, i32, vp]),
    # (cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, accumulate, radii, geom_state, point_list, image_state, grads, dL_dmeans2D, dL_dmeans3D, dL_dlogit_opacities, dL_dcolors_precomp, dL_dshs, dL_dlog_scales, dL_dunnorm_rotations, scratch, scratch_zeroed, have_sh_jacobian, stream)
    "gs_render_backward_raw_grads": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 7 + [i32, i32] + [vp] * 4 + [C.POINTER(GsImageGrads)] + [vp] * 8 + [i32, i32, vp]),
    # (cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, accumulate, radii, geom_state, point_list, image_state, grads, dL_dmeans2D, dL_dmeans3D, dL_dlogit_opacities, dL_dcolors_precomp, dL_dshs, dL_dlog_scales, dL_dunnorm_rotations, scratch, scratch_zeroed, have_sh_jacobian, pose_only, dL_dpose7, pose_scratch, stream)
    "gs_render_backward_raw_pose_grads": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 7 + [i32, i32] + [vp] * 4 + [C.POINTER(GsImageGrads)] + [vp] * 8 + [i32, i32, i32, vp, vp, vp]),
    # (n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, stream)
    "gs_adam_step": (cint, [i64] + [vp] * 4 + [f64] * 4 + [i32, vp]),
    # (count, tensors, stream)
    "gs_adam_step_multi": (cint, [i32, C.POINTER(GsAdamTensor), vp]),
    # (cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, h_pose7, isotropic, radii, geom_state, point_list, image_state, dL_dcolor, dL_ddepth, dL_dmeans2D, scratch, scratch_zeroed, have_sh_jacobian, adam5, stream)
    "gs_render_backward_raw_adam": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 7 + [i32] + [vp] * 8 + [i32, i32, C.POINTER(GsAdamTensor), vp]),
    # (count, tensors, n, n_padded, flat, stream)
    "gs_pack_columns": (cint, [i32, C.POINTER(GsRowTensor), i64, i64, vp, vp]),
    # (count, tensors, row_lo, n_valid, n_rows, grad_shard, out_shard, stream)
    "gs_adam_rows": (cint, [i32, C.POINTER(GsRowTensor), i64, i64, i64, vp, vp, vp]),
    # (count, tensors, n, flat, stream)
    "gs_unpack_columns": (cint, [i32, C.POINTER(GsRowTensor), i64, vp, vp]),
    # (P, isotropic, h_pose7, means3D, unnorm_rotations, logit_opacities, log_scales, out_means3D, out_rotations, out_opacities, out_scales, stream)
    "gs_activate_forward": (cint, [i32, i32] + [vp] * 10),
    # (P, isotropic, h_pose7, unnorm_rotations, out_opacities, out_scales, g_means3D, g_rotations, g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities, d_log_scales, stream)
    "gs_activate_backward": (cint, [i32, i32] + [vp] * 13),
    # (P, isotropic, h_pose7, unnorm_rotations, out_opacities, out_scales, g_means3D, g_rotations, g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities, d_log_scales, stream)
    "gs_activate_backward_accumulate": (cint, [i32, i32] + [vp] * 13),
    # (P, isotropic, h_pose7, means3D, unnorm_rotations, out_opacities, out_scales, g_means3D, g_rotations, g_opacities, g_scales, d_means3D, d_unnorm_rotations, d_logit_opacities, d_log_scales, accumulate, pose_only, dL_dpose7, pose_scratch, stream)
    "gs_activate_backward_pose": (cint, [i32, i32] + [vp] * 13 + [i32, i32, vp, vp, vp]),
    # (width, height)
    "gs_mapping_loss_scratch_bytes": (u64, [i32, i32]),
    # (width, height, im, gt_im, depth, depth_sq, gt_depth, w_im, w_depth, losses, dL_dim, dL_ddepth, scratch, persistent_call, stream)
    "gs_mapping_loss": (cint, [i32, i32] + [vp] * 5 + [f32, f32] + [vp] * 4 + [i64, vp]),
    # (width, height)
    "gs_depth_error_median_scratch_bytes": (u64, [i32, i32]),
    # (width, height, depth, gt_depth, scratch, d_median, stream)
    "gs_depth_error_median": (cint, [i32, i32] + [vp] * 5),
    # (width, height, depth, gt_depth, scratch, d_median, workgroups, stream)
    "gs_depth_error_median_grid": (cint, [i32, i32] + [vp] * 4 + [i32, vp]),
    # (width, height)
    "gs_depth_error_median_workgroups": (i32, [i32, i32]),
    # (width, height, im, gt_im, depth, depth_sq, gt_depth, w_im, w_depth, losses, dL_dim, dL_ddepth, scratch, persistent_call, d_median, stream)
    "gs_mapping_loss_outlier": (cint, [i32, i32] + [vp] * 5 + [f32, f32] + [vp] * 4 + [i64, vp, vp]),
    # (width, height)
    "gs_tracking_loss_scratch_bytes": (u64, [i32, i32]),
    # (width, height, im, gt_im, depth, depth_sq, gt_depth, silhouette, use_sil_for_loss, sil_thres, w_im, w_depth, dL_dim, dL_ddepth, loss_rows, losses, stream)
    "gs_tracking_loss": (cint, [i32, i32] + [vp] * 6 + [i32, f32, f32, f32] + [vp] * 5),
    # (width, height, im, gt_im, depth, depth_sq, gt_depth, silhouette, use_sil_for_loss, sil_thres, w_im, w_depth, dL_dim, dL_ddepth, loss_rows, losses, d_median, stream)
    "gs_tracking_loss_outlier": (cint, [i32, i32] + [vp] * 6 + [i32, f32, f32, f32] + [vp] * 6),
    # (cam, P, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, cam_unnorm_rots, cam_trans, num_frames, time_idx, isotropic, max_2D_radius, seen, radii, geom_state, image_state, d_counts, h_counts, want_backward, stream)
    "gs_preprocess_forward_raw_dev": (cint, [C.POINTER(GsCamera), i32] + [vp] * 8 + [i64, i64, i32] + [vp] * 7 + [i32, vp]),
    # (cam, P, means3D, colors_precomp, logit_opacities, log_scales, unnorm_rotations, isotropic, band_upper, band_lower, radii, geom_state, image_state, d_counts, h_counts, stream)
    "gs_preprocess_forward_topdown": (cint, [C.POINTER(GsCamera), i32] + [vp] * 5 + [i32, f32, f32] + [vp] * 6),
    # (cam, P, D, max_tile_instances, geom_state, bin_state, point_list, image_state, free_opacity, free_map_binary, visible_rgb, visible_map_binary, stream)
    "gs_render_forward_topdown": (cint, [C.POINTER(GsCamera), i32, i64, u32] + [vp] * 9),
    # (cam, P, D, means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, cam_unnorm_rots, cam_trans, num_frames, time_idx, isotropic, radii, geom_state, point_list, image_state, dL_dcolor, dL_ddepth, dL_dmeans2D, scratch, scratch_zeroed, have_sh_jacobian, dL_dpose7, pose_scratch, stream)
    "gs_render_backward_raw_pose_dev": (cint, [C.POINTER(GsCamera), i32, i64] + [vp] * 8 + [i64, i64, i32] + [vp] * 8 + [i32, i32, vp, vp, vp]),
    # ()
    "gs_tracking_state_bytes": (u64, []),
    # (cam_unnorm_rots, cam_trans, num_frames, time_idx, state, stream)
    "gs_tracking_begin": (cint, [vp, vp, i64, i64, vp, vp]),
    # (P, pose_scratch, width, height, loss_rows, w_im, w_depth, cam_unnorm_rots, cam_trans, num_frames, time_idx, lr_rot, lr_trans, step, state, history_row, stream)
    "gs_tracking_step": (cint, [i32, vp, i32, i32, vp, f32, f32, vp, vp, i64, i64, f64, f64, i32, vp, vp, vp]),
    # (n)
    "gs_compact_scratch_bytes": (u64, [i64]),
    # (n, keep, src_index, d_count, scratch, stream)
    "gs_compact_index": (cint, [i64] + [vp] * 5),
    # (n_out, row_floats, src_index, src, dst, stream)
    "gs_gather_rows": (cint, [i64, i32] + [vp] * 4),
    # (n_out, n_copy, row_floats, src_index, src, dst, stream)
    "gs_gather_rows_zero_tail": (cint, [i64, i64, i32] + [vp] * 4),
    # (N, scale_dim, log_scales, logit_opacities, grad_accum, denom, d_scene_radius, grad_thresh, opacity_thresh, remove_big, num_to_split_into, keep_orig, keep_clone, keep_child, split_mask, stream)
    "gs_densify_classify": (cint, [i32, i32] + [vp] * 5 + [f32, f32, i32, i32] + [vp] * 5),
    # (n_child, scale_dim, num_to_split_into, unnorm_rotations, samples, seed, means3D, log_scales, stream)
    "gs_densify_children": (cint, [i32, i32, i32, vp, vp, u64, vp, vp, vp]),
    # (n)
    "gs_compact3_scratch_bytes": (u64, [i64]),
    # (n, keep_a, keep_b, keep_c, repeat_c, src_index, d_counts, scratch, stream)
    "gs_compact_index3": (cint, [i64, vp, vp, vp, i32] + [vp] * 4),
    # (P, radii, seen, max_2D_radius, stream)
    "gs_visibility_stats": (cint, [i32] + [vp] * 4),
    # (P, means2D_grad, seen, grad_accum, denom, stream)
    "gs_accumulate_grad2d": (cint, [i32] + [vp] * 5),
    # (B, H, W, max_clusters, out)
    "gs_grid_dbscan_layout": (cint, [i32] * 4 + [C.POINTER(GsDbscanLayout)]),
    # (B, H, W, values, row_stride, image_stride, threshold, complement, eps, min_samples, max_clusters, workspace, labels, n_clusters, table, sum_value, total, stream)
    "gs_grid_dbscan": (cint, [i32, i32, i32, vp, i64, i64, f32] + [i32] * 4 + [vp] * 7),
    # (B, H, W, max_clusters, max_points, out)
    "gs_cluster_hulls_layout": (cint, [i32] * 5 + [C.POINTER(GsHullLayout)]),
    # (B, H, W, labels, depth, row_stride, image_stride, n_clusters, sum_value, max_clusters, footprint_rows, kh, kw, skip_depth, x_scale, y_scale, max_points, workspace, volume, n_points, contour_xy, sum_volume, sum_invisibility, status, stream)
    "gs_cluster_hulls": (cint, [i32, i32, i32, vp, vp, i64, i64, vp, vp, i32, C.POINTER(u32), i32, i32, f32, f64, f64, i32] + [vp] * 8),
    # (width, height, render_depth, opacity, gt_depth, depth_err_thres, opacity_thres, grid_width, grid_height, mask_full, grid, stream)
    "gs_high_loss_grid": (cint, [i32, i32, vp, vp, vp, f32, f32, i32, i32, vp, vp, vp]),
    # (width, height)
    "gs_grow_scratch_bytes": (u64, [i32, i32]),
    # (width, height, render_depth, silhouette, gt_depth, color, h_intrinsics4, h_c2w12, sil_thres, isotropic, out_means3D, out_rgb_colors, out_unnorm_rotations, out_logit_opacities, out_log_scales, d_counts, scratch, stream)
    "gs_grow_gaussians": (cint, [i32, i32] + [vp] * 6 + [f32, i32] + [vp] * 8),
    # (n_pts, pts_world, n_keyframes, w2c, h_intrinsics9, width, height, edge, counts, stream)
    "gs_keyframe_overlap": (cint, [i32, vp, i32, vp, vp, i32, i32, i32, vp, vp]),
    # (width, height, image, depth, level_value, n_out, h_sizes, color0, depth0, color1, depth1, stream)
    "gs_frame_ingest": (cint, [i32, i32, vp, vp, vp, i32, C.POINTER(i32)] + [vp] * 5),
    # (num_triangles, width, height, capacity, layout)
    "gs_mesh_render_layout": (cint, [i32, i32, i32, u32, C.POINTER(GsMeshLayout)]),
    # (num_vertices, vertices, num_triangles, triangles, vertex_colors, h_intrinsics4, h_w2c12, near_z, width, height, scratch, capacity, depth, tri_id, color, d_counts, stream)
    "gs_mesh_render": (cint, [i32, vp, i32, vp, vp, C.POINTER(f32), C.POINTER(f32), f32, i32, i32, vp, u32, vp, vp, vp, vp, vp]),
    # (num_textures, h_textures, pool_texels)
    "gs_texture_layout": (cint, [i32, C.POINTER(GsTextureDesc), C.POINTER(u64)]),
    # (num_textures, h_textures, textures, pool, pool_texels, stream)
    "gs_texture_build_mips": (cint, [i32, C.POINTER(GsTextureDesc), vp, vp, u64, vp]),
    # (num_vertices, vertices, num_triangles, triangles, vertex_colors, h_intrinsics4, h_w2c12, near_z, width, height, scratch, capacity, depth, tri_id, color, d_counts, uvs, tri_texture, num_textures, h_textures, textures, pool, pool_texels, stream)
    "gs_mesh_render_textured": (cint, [i32, vp, i32, vp, vp, C.POINTER(f32), C.POINTER(f32), f32, i32, i32, vp, u32, vp, vp, vp, vp, vp, vp, i32,
                                       C.POINTER(GsTextureDesc), vp, vp, u64, vp]),
    # (num_triangles, grid_width, grid_height, capacity, layout)
    "gs_mesh_navgrid_layout": (cint, [i32, i32, i32, u32, C.POINTER(GsMeshLayout)]),
    # (num_vertices, vertices, num_triangles, triangles, x0, z0, cell, floor_y, max_climb, agent_height, grid_width, grid_height, scratch, capacity, grid, d_counts, stream)
    "gs_mesh_navgrid": (cint, [i32, vp, i32, vp, f64, f64, f64, f64, f64, f64, i32, i32, vp, u32, vp, vp, vp]),
    # (width, height, depth, h_intrinsics4, h_c2w12, points, valid, stream)
    "gs_depth_cloud": (cint, [i32, i32, vp, C.POINTER(f32), C.POINTER(f32), vp, vp, vp]),
    # (n_query, n_points)
    "gs_cloud_nearest_scratch_bytes": (u64, [i64, i64]),
    # (n_query, query, query_valid, n_points, points, points_valid, flags, out, scratch, stream)
    "gs_cloud_nearest": (cint, [i64, vp, vp, i64, vp, vp, i32, vp, vp, vp]),
    # ()
    "gs_completion_row_scratch_bytes": (u64, []),
    # (n_samples, min_dist, n_acc, acc_dist, acc_valid, path_length, row6, scratch, stream)
    "gs_completion_row": (cint, [i64, vp, i64, vp, vp, f64, vp, vp, vp]),
    # (width, height, flags, layout)
    "gs_eval_frame_layout": (cint, [i32, i32, i32, C.POINTER(GsEvalLayout)]),
    # (width, height, im, depth, silhouette, gt_im, gt_depth, sil_thres, flags, row, scratch, stream)
    "gs_eval_frame": (cint, [i32, i32] + [vp] * 5 + [f32, i32, vp, vp, vp]),
    # (nx, ny, nz, h_origin3, voxel_size, trunc, max_weight, tsdf, weight, color, n_frames, width, height, depth, frame_color, silhouette, h_intrinsics4, h_w2c12, sil_thres, depth_max, stream)
    "gs_tsdf_integrate": (cint, [i32, i32, i32, C.POINTER(f32), f32, f32, f32, vp, vp, vp, i32, i32, i32, vp, vp, vp, C.POINTER(f32), C.POINTER(f32), f32, f32, vp]),
    # (nx, ny, nz)
    "gs_tsdf_extract_scratch_bytes": (u64, [i32, i32, i32]),
    # (nx, ny, nz, tsdf, weight, min_weight, scratch, d_counts, stream)
    "gs_tsdf_count": (cint, [i32, i32, i32, vp, vp, f32, vp, vp, vp]),
    # (nx, ny, nz, h_origin3, voxel_size, tsdf, color, scratch, max_vertices, max_triangles, vertices, vertex_colors, triangles, stream)
    "gs_tsdf_emit": (cint, [i32, i32, i32, C.POINTER(f32), f32, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    # (H, W)
    "gs_roadmap_scratch_bytes": (u64, [i32, i32]),
    # (H, W, free_map, unseen, agent_r, agent_c, open_size, dilate, trav, scratch, d_status, stream)
    "gs_traversable_map": (cint, [i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    # (H, W, trav, dist2, feature, scratch, stream)
    "gs_clearance_field": (cint, [i32, i32, vp, vp, vp, vp, vp]),
    # (H, W, trav, dist2, feature, min_dist2, gamma2, roadmap, stream)
    "gs_voronoi_roadmap": (cint, [i32, i32, vp, vp, vp, i32, i32, vp, vp]),
    # (H, W, mask, seed_r, seed_c, d_seed_rc, field, scratch, d_status, h_rounds, stream)
    "gs_grid_geodesic": (cint, [i32, i32, vp, i32, i32, vp, vp, vp, vp, C.POINTER(i32), vp]),
    # (H, W, roadmap, field, d_entry4, scratch, stream)
    "gs_roadmap_entry": (cint, [i32, i32, vp, vp, vp, vp, vp]),
    # (H, W, roadmap, dist2, field, cell, node_rc, node_dist2, node_field, d_count, scratch, stream)
    "gs_roadmap_nodes": (cint, [i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    # (H, W, mask, field, target_r, target_c, d_target_rc, capacity, path_rc, d_count2, stream)
    "gs_trace_path": (cint, [i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp]),
    # (path)
    "gs_set_node_distance_path": (cint, [i32]),
    # (H, W)
    "gs_node_distances_scratch_bytes": (u64, [i32, i32]),
    # (H, W, roadmap, K, node_rc, D, scratch, stream)
    "gs_node_distances": (cint, [i32, i32, vp, i32, vp, vp, vp, vp]),
    # (H, W, dist2, n, segments, clearance, stream)
    "gs_segment_clearance": (cint, [i32, i32, vp, i32, vp, vp, vp]),
    # (K)
    "gs_subregions_scratch_bytes": (u64, [i32]),
    # (K, node_rc, D, path_weight, coord_weight, threshold, labels, d_count, heights, scratch, stream)
    "gs_subregions": (cint, [i32, vp, vp, f64, f64, f64, vp, vp, vp, vp, vp]),
}

SYMBOLS = tuple(BINDINGS)


def _bind(lib):
    # a stale prebuilt library (another round's .so, an old emulated build) must fail HERE, not misread pointers later
    try:
        lib.gs_abi_version.restype = i32
        have = int(lib.gs_abi_version())
    except AttributeError:
        have = None
    if have != ABI_VERSION:
        raise RuntimeError(f"{getattr(lib, '_name', 'library')}: C ABI version {have}, this binding needs {ABI_VERSION} (include/gsplat_hip.h "
                           "GS_ABI_VERSION) -- rebuild it: python -c 'import __graft_entry__ as g; g.build()'")
    for name, (restype, argtypes) in BINDINGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def get():
    """The HIP library; raises loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). activesplat_amd has no CPU fallback.")
        _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


def load_for_tests(path: str):
    """TEST HOOK ONLY: bind an alternative build of the same C ABI (the host-emulated kernels)."""
    global _lib, _emulated, _status
    _lib = _bind(C.CDLL(path))
    _emulated = True
    _status = None
    return _lib


def unload_for_tests():
    global _lib, _emulated, _status
    _lib = None
    _emulated = False
    _status = None


#: the library's host-mapped status word (gs_async_status_word), as a ctypes view: a plain host load per poll
_status = None


def poll_async_status():
    """Called in front of every render: has a chained backward walk of an EARLIER launch run out of its bounded wait (include/gsplat_hip.h,
    gs_set_backward_chain_polls)?  Then that backward's gradients hold NaNs: the word is cleared, chaining is switched off for the rest of the
    process (every quadrant walked by one wavefront again: slower at 640 x 480, no hand-over to wait for) and the caller is told."""
    global _status
    if _status is None:
        w = C.POINTER(C.c_uint32)()
        check(get().gs_async_status_word(C.byref(w)))
        _status = w
    if _status[0]:
        check(get().gs_set_backward_chain(1, -1))
        check(get().gs_async_status_clear())      # (synchronises the device, then clears the sticky device word: optimiser steps run again)
        _status[0] = 0
        raise RuntimeError("activesplat_amd: a chained backward walk timed out waiting for the piece in front of it -- the gradients of the previous "
                           "backward on this process are invalid (NaN); optimiser steps enqueued behind it were SKIPPED by their kernels (parameters and "
                           "moments untouched, step counters one ahead).  Chained walks are now off (gs_set_backward_chain(1, -1)); render that frame again.")


def emulated() -> bool:
    return _emulated


def check(rc: int):
    if rc != 0:
        raise Exception(get().gs_last_error().decode())


_raw_stream = None


def stream_handle(device) -> int:
    """The current HIP stream of `device` as an integer handle (0 for the host-emulated test build).  torch.cuda.current_stream()
    builds a Stream object per call (~6 us; a mapping iteration asks seven times): the raw accessor returns the same handle in a
    fraction of a microsecond.  Falls back to the public call if this torch build does not have it."""
    global _raw_stream
    if device.type != "cuda":
        return 0
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if _raw_stream:
        return int(_raw_stream(idx))
    return int(torch.cuda.current_stream(device).cuda_stream)


def stream_ptr(device):
    return C.c_void_p(stream_handle(device))


def profile_collect():
    """-> {stage_name: (total_ms, calls)} since gs_profile_enable(1); synchronises the recorded events."""
    lib = get()
    n = lib.gs_profile_stage_count()
    ms = (C.c_float * n)()
    calls = (C.c_int32 * n)()
    check(lib.gs_profile_collect(ms, calls, n))
    return {lib.gs_profile_stage_name(i).decode(): (float(ms[i]), int(calls[i])) for i in range(n)}
