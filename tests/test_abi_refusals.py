"""CPU: every argument refusal of the C ABI (csrc/api.hip), by return code and gs_last_error text, against the real gfx950 library and the
host-emulated build of the same sources.  A refused call returns before the first HIP runtime call, so none of this needs a GPU.

REFUSALS is the table: (entry point, arguments, return code, gs_last_error text).  The arguments are given by NAME, as the prototype in
include/gsplat_hip.h names them, on top of that entry point's PLAUSIBLE call (below): every pointer the address of a small host buffer (never
dereferenced by a refused call; the host-side arrays -- camera, pose, descriptors, sizes, footprint -- are real), every count 1, every flag 0.
Every row must be refused; the text must be the library's to the byte.

Coverage: 119 of the 122 GS_EINVAL / GS_ECAPACITY sites of api.hip, every distinct text they can produce, and the three alignment refusals
(fail_adam_alignment).  None sits behind a HIP runtime call.  Left out, because no argument list reaches them through the C ABI (each entry
point checks the same condition first, or never passes the combination):
  - "gs_render_backward_raw_pose: raw-parameter mode with a pose-gradient output and its scratch only"
  - "gs_render_backward_raw_pose_dev: the pose-only backward only"
  - "gs_render_backward_raw_adam: raw-parameter mode without accumulation only"
and one text of a shared site: "gs_eval_frame_layout: GS_EVAL_MS_SSIM needs ..." (the layout call answers that question instead of refusing).
"""
import ctypes as C
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = 1, 3

_mem = (C.c_char * 1024)()
BUF = (C.addressof(_mem) + 63) // 64 * 64          # a 64-byte aligned host address with room behind it
POSE = (C.c_float * 7)(1, 0, 0, 0, 0, 0, 0)
ZERO_BY_DEFAULT = {"isotropic", "accumulate", "pose_only", "complement", "remove_big", "use_sil_for_loss", "scratch_zeroed", "have_sh_jacobian",
                   "want_backward", "persistent_call", "time_idx", "row_lo", "image_stride", "edge", "workgroups", "seed", "flags", "on"}
ALIGN = "param / grad / exp_avg / exp_avg_sq must be 16-byte aligned (the kernel makes 128-bit accesses)"
DBSCAN = "size out of range (1 <= B <= 65535, H, W <= 4096, H * W <= 65536, 1 <= max_clusters <= 65535"


def cam(width=32, height=32, views=1, sh_degree=0, sh_coeffs=0, tanfovx=1.0):
    from activesplat_amd import _lib
    return C.pointer(_lib.GsCamera(width, height, sh_degree, sh_coeffs, tanfovx, 1.0, 1.0, views, BUF, BUF, BUF, BUF))


def adam5(params=(BUF,) * 5, widths=(3, 1, 3, 4, 3), P=1):
    from activesplat_amd import _lib
    return (_lib.GsAdamTensor * 5)(*[_lib.GsAdamTensor(w * P, p, BUF, BUF, BUF, 1e-3, 0.9, 0.999, 1e-8, 1, 0) for p, w in zip(params, widths)])


def adam_tensors(*rows):
    """rows of (n, param, step)"""
    from activesplat_amd import _lib
    return (_lib.GsAdamTensor * len(rows))(*[_lib.GsAdamTensor(n, p, BUF, BUF, BUF, 1e-3, 0.9, 0.999, 1e-8, step, 0) for n, p, step in rows])


def row_tensors():
    from activesplat_amd import _lib
    return (_lib.GsRowTensor * 1)(_lib.GsRowTensor(BUF, BUF, BUF, BUF, 1e-3, 0.9, 0.999, 1e-8, 1, 1))


# the plausible call of an entry point, where "every pointer a buffer, every count 1, every flag 0" is not one
PLAUSIBLE = {
    "gs_preprocess_forward": dict(shs=None, cov3D_precomp=None),
    "gs_preprocess_forward_raw": dict(shs=None, h_pose7=POSE),
    "gs_preprocess_forward_raw_dev": dict(shs=None),
    "gs_render_backward": dict(shs=None, dL_dshs=None, cov3D_precomp=None, dL_dcov3D=None),
    "gs_render_backward_raw": dict(shs=None, dL_dshs=None, h_pose7=POSE),
    "gs_render_backward_raw_pose": dict(shs=None, dL_dshs=None, h_pose7=POSE),
    "gs_render_backward_raw_pose_dev": dict(shs=None),
    "gs_render_backward_raw_adam": dict(shs=None, h_pose7=POSE, adam5=adam5),
    "gs_adam_step_multi": dict(tensors=lambda: adam_tensors((4, BUF, 1))),
    "gs_pack_columns": dict(tensors=row_tensors),
    "gs_adam_rows": dict(tensors=row_tensors),
    "gs_unpack_columns": dict(tensors=row_tensors),
    "gs_activate_forward": dict(h_pose7=POSE),
    "gs_activate_backward": dict(h_pose7=POSE),
    "gs_activate_backward_accumulate": dict(h_pose7=POSE),
    "gs_activate_backward_pose": dict(h_pose7=POSE),
    "gs_cluster_hulls_layout": dict(max_points=4),
    "gs_cluster_hulls": dict(max_points=4, footprint_rows=lambda: (C.c_uint32 * 15)(1)),
    "gs_frame_ingest": dict(h_sizes=lambda: (C.c_int32 * 4)(1, 1, 1, 1)),
    "gs_depth_cloud": dict(h_intrinsics4=lambda: (C.c_float * 4)(1, 1, 0, 0)),
    "gs_profile_collect": dict(n_stages=64),
}

REFUSALS = [
    ("gs_profile_collect", dict(calls=None), EINVAL, "gs_profile_collect: bad argument"),
    ("gs_profile_collect", dict(n_stages=1), EINVAL, "gs_profile_collect: bad argument"),
    ("gs_set_sort_path", dict(path=3), EINVAL, "gs_set_sort_path: bad path"),
    ("gs_set_backward_chain", dict(pieces=0), EINVAL, "gs_set_backward_chain: pieces out of range"),
    ("gs_set_backward_chain", dict(pieces=4), EINVAL, "gs_set_backward_chain: pieces out of range"),
    ("gs_set_backward_segments", dict(segments=4), EINVAL, "gs_set_backward_segments: 1, 2 or 3"),
    ("gs_atlas_layout", dict(num_views=65), EINVAL, "gs_atlas_layout: bad argument"),
    ("gs_geom_layout", dict(P=-1), EINVAL, "gs_geom_layout: bad argument"),
    ("gs_geom_layout", dict(out=None), EINVAL, "gs_geom_layout: bad argument"),
    ("gs_image_layout", dict(width=0), EINVAL, "gs_image_layout: bad argument"),
    ("gs_bin_layout", dict(D=-1), EINVAL, "gs_bin_layout: bad argument"),
    # the per-Gaussian forward
    ("gs_preprocess_forward", dict(cam=None), EINVAL, "gs_preprocess_forward: invalid camera settings"),
    ("gs_preprocess_forward", dict(cam=lambda: cam(tanfovx=0.0)), EINVAL, "gs_preprocess_forward: invalid camera settings"),
    ("gs_preprocess_forward", dict(cam=lambda: cam(views=65)), EINVAL, "gs_preprocess_forward: invalid camera settings"),
    ("gs_preprocess_forward", dict(geom_state=None), EINVAL, "gs_preprocess_forward: null state pointer"),
    ("gs_preprocess_forward", dict(P=-1), EINVAL, "gs_preprocess_forward: null state pointer"),
    ("gs_preprocess_forward", dict(means3D=None), EINVAL, "gs_preprocess_forward: null input pointer"),
    ("gs_preprocess_forward", dict(colors_precomp=None), EINVAL, "Please provide excatly one of either SHs or precomputed colors!"),
    ("gs_preprocess_forward", dict(shs=BUF), EINVAL, "Please provide excatly one of either SHs or precomputed colors!"),
    ("gs_preprocess_forward", dict(cov3D_precomp=BUF), EINVAL,
     "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"),
    ("gs_preprocess_forward", dict(rotations=None), EINVAL, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"),
    ("gs_preprocess_forward", dict(shs=BUF, colors_precomp=None, cam=lambda: cam(sh_degree=1, sh_coeffs=1)), EINVAL,
     "gs_preprocess_forward: sh_degree / sh_coeffs / campos inconsistent"),
    ("gs_preprocess_forward_raw", dict(h_pose7=None), EINVAL, "gs_preprocess_forward_raw: null pose"),
    ("gs_preprocess_forward_raw", dict(cam=lambda: cam(views=2)), EINVAL, "gs_preprocess_forward_raw: one view only"),
    ("gs_preprocess_forward_raw", dict(shs=BUF, colors_precomp=None, cam=lambda: cam(sh_degree=2, sh_coeffs=9)), EINVAL,
     "gs_preprocess_forward_raw: scale / rotation parameters with colours or 16-coefficient SH rows only"),
    ("gs_preprocess_forward_raw", dict(d_counts=None), EINVAL, "gs_preprocess_forward: null state pointer"),
    ("gs_preprocess_forward_raw", dict(colors_precomp=None), EINVAL, "Please provide excatly one of either SHs or precomputed colors!"),
    ("gs_preprocess_forward_raw_dev", dict(time_idx=1), EINVAL,
     "gs_preprocess_forward_raw_dev: null pose columns or time index outside [0, num_frames)"),
    ("gs_preprocess_forward_raw_dev", dict(cam_trans=None), EINVAL,
     "gs_preprocess_forward_raw_dev: null pose columns or time index outside [0, num_frames)"),
    ("gs_preprocess_forward_raw_dev", dict(log_scales=None), EINVAL, "gs_preprocess_forward_raw_dev: null scale / rotation parameters"),
    ("gs_preprocess_forward_raw_dev", dict(cam=lambda: cam(views=2)), EINVAL, "gs_preprocess_forward_raw: one view only"),
    ("gs_preprocess_forward_raw_dev", dict(image_state=None), EINVAL, "gs_preprocess_forward: null state pointer"),
    ("gs_preprocess_forward_topdown", dict(cam=lambda: cam(views=2)), EINVAL, "gs_preprocess_forward_topdown: one view only"),
    ("gs_preprocess_forward_topdown", dict(colors_precomp=None), EINVAL, "gs_preprocess_forward_topdown: null colour / scale / rotation parameters"),
    ("gs_preprocess_forward_topdown", dict(band_upper=math.nan), EINVAL, "gs_preprocess_forward_topdown: NaN height band"),
    ("gs_preprocess_forward_topdown", dict(cam=None), EINVAL, "gs_preprocess_forward: invalid camera settings"),
    ("gs_preprocess_forward_topdown", dict(radii=None), EINVAL, "gs_preprocess_forward: null input pointer"),
    # the forward blend
    ("gs_render_forward", dict(cam=None), EINVAL, "gs_render_forward: invalid camera settings"),
    ("gs_render_forward", dict(out_color=None), EINVAL, "gs_render_forward: null pointer"),
    ("gs_render_forward", dict(bin_state=None), EINVAL, "gs_render_forward: null binning workspace"),
    ("gs_render_forward", dict(D=1 << 32), ECAPACITY, "gs_render_forward: more than 2^32 tile instances"),
    ("gs_render_forward_topdown", dict(cam=None), EINVAL, "gs_render_forward_topdown: invalid camera settings"),
    ("gs_render_forward_topdown", dict(cam=lambda: cam(views=2)), EINVAL, "gs_render_forward_topdown: one view only"),
    ("gs_render_forward_topdown", dict(free_opacity=None), EINVAL, "gs_render_forward_topdown: null pointer"),
    ("gs_render_forward_topdown", dict(visible_rgb=BUF + 1), EINVAL, "gs_render_forward_topdown: output maps must be 4-byte aligned"),
    ("gs_render_forward_topdown", dict(point_list=None), EINVAL, "gs_render_forward_topdown: null binning workspace"),
    ("gs_render_forward_topdown", dict(D=1 << 32), ECAPACITY, "gs_render_forward_topdown: more than 2^32 tile instances"),
    # the backward: plain, raw, raw + pose gradient, device pose, fused Adam
    ("gs_render_backward", dict(cam=None), EINVAL, "gs_render_backward: invalid camera settings"),
    ("gs_render_backward", dict(cam=lambda: cam(views=2)), EINVAL, "gs_render_backward: multi-view atlas renders are forward-only"),
    ("gs_render_backward", dict(scratch=None), EINVAL, "gs_render_backward: null pointer"),
    ("gs_render_backward", dict(D=-1), EINVAL, "gs_render_backward: null pointer"),
    ("gs_render_backward", dict(means3D=None), EINVAL, "gs_render_backward: null input/output pointer"),
    ("gs_render_backward", dict(dL_dopacities=None), EINVAL, "gs_render_backward: null input/output pointer"),
    ("gs_render_backward", dict(dL_dcolors_precomp=None), EINVAL, "gs_render_backward: missing colour gradient output"),
    ("gs_render_backward", dict(shs=BUF), EINVAL, "gs_render_backward: missing colour gradient output"),
    ("gs_render_backward", dict(dL_dscales=None), EINVAL, "gs_render_backward: missing covariance inputs/outputs"),
    ("gs_render_backward", dict(cov3D_precomp=BUF), EINVAL, "gs_render_backward: missing covariance inputs/outputs"),
    ("gs_render_backward_raw", dict(h_pose7=None), EINVAL, "gs_render_backward_raw: null pose / opacity parameters"),
    ("gs_render_backward_raw", dict(logit_opacities=None), EINVAL, "gs_render_backward_raw: null pose / opacity parameters"),
    ("gs_render_backward_raw", dict(cam=lambda: cam(views=2)), EINVAL, "gs_render_backward_raw: one view only"),
    ("gs_render_backward_raw", dict(shs=BUF, colors_precomp=None, cam=lambda: cam(sh_degree=2, sh_coeffs=9)), EINVAL,
     "gs_render_backward_raw: scale / rotation parameters with colours or 16-coefficient SH rows only"),
    ("gs_render_backward_raw", dict(P=0, logit_opacities=None), EINVAL,
     "gs_render_backward_raw: scale / rotation parameters with colours or 16-coefficient SH rows only"),
    ("gs_render_backward_raw", dict(cam=None), EINVAL, "gs_render_backward: invalid camera settings"),
    ("gs_render_backward_raw", dict(dL_dcolor=None), EINVAL, "gs_render_backward: null pointer"),
    ("gs_render_backward_raw", dict(dL_dmeans3D=None), EINVAL, "gs_render_backward: null input/output pointer"),
    ("gs_render_backward_raw", dict(dL_dunnorm_rotations=None), EINVAL, "gs_render_backward: missing covariance inputs/outputs"),
    ("gs_render_backward_raw_pose", dict(h_pose7=None), EINVAL, "gs_render_backward_raw_pose: null pose / opacity parameters"),
    ("gs_render_backward_raw_pose", dict(dL_dpose7=None), EINVAL, "gs_render_backward_raw_pose: null pose-gradient output or scratch"),
    ("gs_render_backward_raw_pose", dict(pose_scratch=None), EINVAL, "gs_render_backward_raw_pose: null pose-gradient output or scratch"),
    ("gs_render_backward_raw_pose", dict(pose_only=1, means3D=None), EINVAL, "gs_render_backward_raw_pose: null input/output pointer"),
    ("gs_render_backward_raw_pose", dict(pose_only=0, dL_dmeans3D=None), EINVAL, "gs_render_backward: null input/output pointer"),
    ("gs_render_backward_raw_pose", dict(cam=lambda: cam(views=2)), EINVAL, "gs_render_backward_raw: one view only"),
    ("gs_render_backward_raw_pose_dev", dict(cam_unnorm_rots=None), EINVAL,
     "gs_render_backward_raw_pose_dev: null pose columns or time index outside [0, num_frames)"),
    ("gs_render_backward_raw_pose_dev", dict(time_idx=-1), EINVAL,
     "gs_render_backward_raw_pose_dev: null pose columns or time index outside [0, num_frames)"),
    ("gs_render_backward_raw_pose_dev", dict(logit_opacities=None), EINVAL, "gs_render_backward_raw_pose_dev: null opacity parameters"),
    ("gs_render_backward_raw_pose_dev", dict(pose_scratch=None), EINVAL, "gs_render_backward_raw_pose_dev: null pose scratch"),
    ("gs_render_backward_raw_pose_dev", dict(dL_dmeans2D=None), EINVAL, "gs_render_backward_raw_pose: null input/output pointer"),
    ("gs_render_backward_raw_pose_dev", dict(geom_state=None), EINVAL, "gs_render_backward: null pointer"),
    ("gs_render_backward_raw_adam", dict(adam5=None), EINVAL, "gs_render_backward_raw_adam: null pose / opacity parameters / descriptors"),
    ("gs_render_backward_raw_adam", dict(dL_dmeans2D=None), EINVAL, "gs_render_backward_raw_adam: null input/output pointer"),
    ("gs_render_backward_raw_adam", dict(colors_precomp=None), EINVAL, "gs_render_backward_raw_adam: null input/output pointer"),
    ("gs_render_backward_raw_adam", dict(shs=BUF, colors_precomp=None, cam=lambda: cam(sh_degree=3, sh_coeffs=16)), EINVAL,
     "gs_render_backward_raw_adam: SH rows need the forward's saved Jacobian (have_sh_jacobian = 1)"),
    ("gs_render_backward_raw_adam", dict(adam5=lambda: adam5(params=(BUF + 64, BUF, BUF, BUF, BUF))), EINVAL,
     "gs_render_backward_raw_adam: descriptor of means3D does not describe the input tensor (param / moments / n / step)"),
    ("gs_render_backward_raw_adam", dict(adam5=lambda: adam5(widths=(3, 2, 3, 4, 3))), EINVAL,
     "gs_render_backward_raw_adam: descriptor of logit_opacities does not describe the input tensor (param / moments / n / step)"),
    ("gs_render_backward_raw_adam", dict(isotropic=1), EINVAL,
     "gs_render_backward_raw_adam: descriptor of log_scales does not describe the input tensor (param / moments / n / step)"),
    ("gs_render_backward_raw_adam", dict(adam5=lambda: adam5(widths=(3, 1, 3, 3, 3))), EINVAL,
     "gs_render_backward_raw_adam: descriptor of unnorm_rotations does not describe the input tensor (param / moments / n / step)"),
    ("gs_render_backward_raw_adam", dict(adam5=lambda: adam5(widths=(3, 1, 3, 4, 48))), EINVAL,
     "gs_render_backward_raw_adam: descriptor of the colours does not describe the input tensor (param / moments / n / step)"),
    ("gs_render_backward_raw_adam", dict(unnorm_rotations=BUF + 4, adam5=lambda: adam5(params=(BUF, BUF, BUF, BUF + 4, BUF))), EINVAL,
     "gs_render_backward_raw_adam: tensor 3: " + ALIGN),
    ("gs_render_backward_raw_adam", dict(cam=lambda: cam(views=2)), EINVAL, "gs_render_backward_raw: one view only"),
    # tracking
    ("gs_tracking_loss", dict(width=0), EINVAL, "gs_tracking_loss: bad image size"),
    ("gs_tracking_loss", dict(width=65536, height=32768), EINVAL, "gs_tracking_loss: bad image size"),
    ("gs_tracking_loss", dict(im=None), EINVAL, "gs_tracking_loss: null pointer"),
    ("gs_tracking_loss", dict(use_sil_for_loss=1, silhouette=None), EINVAL, "gs_tracking_loss: null pointer"),
    ("gs_tracking_loss_outlier", dict(height=0), EINVAL, "gs_tracking_loss_outlier: bad image size"),
    ("gs_tracking_loss_outlier", dict(d_median=None), EINVAL, "gs_tracking_loss_outlier: null pointer"),
    ("gs_tracking_loss_outlier", dict(loss_rows=None), EINVAL, "gs_tracking_loss_outlier: null pointer"),
    ("gs_tracking_begin", dict(state=None), EINVAL, "gs_tracking_begin: null pointer or time index outside [0, num_frames)"),
    ("gs_tracking_begin", dict(num_frames=0), EINVAL, "gs_tracking_begin: null pointer or time index outside [0, num_frames)"),
    ("gs_tracking_step", dict(loss_rows=None), EINVAL, "gs_tracking_step: null pointer or time index outside [0, num_frames)"),
    ("gs_tracking_step", dict(step=0), EINVAL, "gs_tracking_step: bad size or step (the first step is 1)"),
    # optimiser
    ("gs_adam_step", dict(step=0), EINVAL, "gs_adam_step: bad n/step"),
    ("gs_adam_step", dict(grad=None), EINVAL, "gs_adam_step: null pointer"),
    ("gs_adam_step", dict(exp_avg=BUF + 8), EINVAL, "gs_adam_step: tensor 0: " + ALIGN),
    ("gs_adam_step_multi", dict(count=-1), EINVAL, "gs_adam_step_multi: bad count/tensors"),
    ("gs_adam_step_multi", dict(tensors=None), EINVAL, "gs_adam_step_multi: bad count/tensors"),
    ("gs_adam_step_multi", dict(tensors=lambda: adam_tensors((4, BUF, 0))), EINVAL, "gs_adam_step_multi: a tensor has bad n/step"),
    ("gs_adam_step_multi", dict(tensors=lambda: adam_tensors((4, None, 1))), EINVAL, "gs_adam_step_multi: a tensor has a null pointer"),
    ("gs_adam_step_multi", dict(count=2, tensors=lambda: adam_tensors((4, BUF, 1), (4, BUF + 4, 1))), EINVAL, "gs_adam_step_multi: tensor 1: " + ALIGN),
    ("gs_pack_columns", dict(count=0), EINVAL, "gs_pack_columns: bad argument"),
    ("gs_pack_columns", dict(n_padded=0), EINVAL, "gs_pack_columns: bad argument"),
    ("gs_adam_rows", dict(count=17), EINVAL, "gs_adam_rows: bad argument"),
    ("gs_adam_rows", dict(grad_shard=None), EINVAL, "gs_adam_rows: bad argument"),
    ("gs_unpack_columns", dict(tensors=None), EINVAL, "gs_unpack_columns: bad argument"),
    ("gs_activate_forward", dict(P=-1), EINVAL, "gs_activate_forward: bad argument"),
    ("gs_activate_forward", dict(out_scales=None), EINVAL, "gs_activate_forward: bad argument"),
    ("gs_activate_backward", dict(h_pose7=None), EINVAL, "gs_activate_backward: bad argument"),
    ("gs_activate_backward_accumulate", dict(d_log_scales=None), EINVAL, "gs_activate_backward_accumulate: bad argument"),
    ("gs_activate_backward_pose", dict(dL_dpose7=None), EINVAL, "gs_activate_backward_pose: bad argument"),
    ("gs_activate_backward_pose", dict(pose_only=0, d_means3D=None), EINVAL, "gs_activate_backward_pose: bad argument"),
    # losses
    ("gs_mapping_loss", dict(width=0), EINVAL, "gs_mapping_loss: bad argument"),
    ("gs_mapping_loss", dict(persistent_call=-1), EINVAL, "gs_mapping_loss: bad argument"),
    ("gs_mapping_loss_outlier", dict(d_median=None), EINVAL, "gs_mapping_loss_outlier: bad argument"),
    ("gs_mapping_loss_outlier", dict(losses=None), EINVAL, "gs_mapping_loss_outlier: bad argument"),
    ("gs_depth_error_median", dict(width=0), EINVAL, "gs_depth_error_median: bad image size"),
    ("gs_depth_error_median", dict(d_median=None), EINVAL, "gs_depth_error_median: null pointer"),
    ("gs_depth_error_median_grid", dict(width=65536, height=32768), EINVAL, "gs_depth_error_median: bad image size"),
    ("gs_depth_error_median_grid", dict(scratch=None), EINVAL, "gs_depth_error_median: null pointer"),
    ("gs_depth_error_median_grid", dict(workgroups=1025), EINVAL, "gs_depth_error_median_grid: 0 (automatic) .. 1024 workgroups"),
    # map surgery
    ("gs_compact_index", dict(keep=None), EINVAL, "gs_compact_index: bad argument"),
    ("gs_compact_index", dict(n=1 << 32), ECAPACITY, "gs_compact_index: more than 2^32 rows"),
    ("gs_compact_index3", dict(repeat_c=0), EINVAL, "gs_compact_index3: bad argument"),
    ("gs_compact_index3", dict(n=1 << 31), ECAPACITY, "gs_compact_index3: more than 2^32 rows"),
    ("gs_gather_rows", dict(row_floats=0), EINVAL, "gs_gather_rows: bad argument"),
    ("gs_gather_rows_zero_tail", dict(n_copy=2), EINVAL, "gs_gather_rows_zero_tail: bad argument"),
    ("gs_densify_classify", dict(scale_dim=2), EINVAL, "gs_densify_classify: bad argument"),
    ("gs_densify_classify", dict(denom=None), EINVAL, "gs_densify_classify: bad argument"),
    ("gs_densify_children", dict(num_to_split_into=0), EINVAL, "gs_densify_children: bad argument"),
    ("gs_visibility_stats", dict(radii=None), EINVAL, "gs_visibility_stats: bad argument"),
    ("gs_accumulate_grad2d", dict(seen=None), EINVAL, "gs_accumulate_grad2d: bad argument"),
    # planner: clustering, hulls, high-loss grid
    ("gs_grid_dbscan_layout", dict(B=0), EINVAL, "gs_grid_dbscan_layout: " + DBSCAN + ")"),
    ("gs_grid_dbscan_layout", dict(out=None), EINVAL, "gs_grid_dbscan_layout: " + DBSCAN + ")"),
    ("gs_grid_dbscan", dict(H=4097), EINVAL, "gs_grid_dbscan: " + DBSCAN + ")"),
    ("gs_grid_dbscan", dict(eps=9), EINVAL, "gs_grid_dbscan: eps must be 1..8 and min_samples at least 1"),
    ("gs_grid_dbscan", dict(values=None), EINVAL, "gs_grid_dbscan: null pointer, workspace not 8-byte aligned, or row_stride below W"),
    ("gs_grid_dbscan", dict(workspace=BUF + 4), EINVAL, "gs_grid_dbscan: null pointer, workspace not 8-byte aligned, or row_stride below W"),
    ("gs_grid_dbscan", dict(W=2), EINVAL, "gs_grid_dbscan: null pointer, workspace not 8-byte aligned, or row_stride below W"),
    ("gs_cluster_hulls_layout", dict(max_points=3), EINVAL, "gs_cluster_hulls_layout: " + DBSCAN + ", 4 <= max_points <= 4096)"),
    ("gs_cluster_hulls", dict(max_points=4097), EINVAL, "gs_cluster_hulls: " + DBSCAN + ", 4 <= max_points <= 4096)"),
    ("gs_cluster_hulls", dict(kh=2), EINVAL, "gs_cluster_hulls: the footprint must have odd kh and kw in 1..15"),
    ("gs_cluster_hulls", dict(footprint_rows=None), EINVAL, "gs_cluster_hulls: the footprint must have odd kh and kw in 1..15"),
    ("gs_cluster_hulls", dict(footprint_rows=lambda: (C.c_uint32 * 15)(2)), EINVAL, "gs_cluster_hulls: a footprint row has a cell at or beyond kw"),
    ("gs_cluster_hulls", dict(status=None), EINVAL,
     "gs_cluster_hulls: null pointer (only contour_xy may be null), workspace not 8-byte aligned, or row_stride below W"),
    ("gs_cluster_hulls", dict(x_scale=math.inf), EINVAL, "gs_cluster_hulls: x_scale and y_scale must be finite"),
    ("gs_cluster_hulls", dict(y_scale=math.nan), EINVAL, "gs_cluster_hulls: x_scale and y_scale must be finite"),
    ("gs_high_loss_grid", dict(width=16385), EINVAL, "gs_high_loss_grid: image size out of range (1 <= width, height <= 16384)"),
    ("gs_high_loss_grid", dict(grid_width=0), EINVAL,
     "gs_high_loss_grid: grid size out of range (1 <= grid_width, grid_height <= 4096, grid_width * grid_height <= 65536)"),
    ("gs_high_loss_grid", dict(depth_err_thres=-1.0), EINVAL, "gs_high_loss_grid: thresholds must be finite and not negative"),
    ("gs_high_loss_grid", dict(opacity_thres=math.nan), EINVAL, "gs_high_loss_grid: thresholds must be finite and not negative"),
    ("gs_high_loss_grid", dict(grid=None), EINVAL, "gs_high_loss_grid: null pointer (only mask_full may be null)"),
    # map growth, keyframes, ingest
    ("gs_grow_gaussians", dict(color=None), EINVAL, "gs_grow_gaussians: bad argument"),
    ("gs_grow_gaussians", dict(width=65536, height=32768), EINVAL, "gs_grow_gaussians: bad image size"),
    ("gs_keyframe_overlap", dict(h_intrinsics9=None), EINVAL, "gs_keyframe_overlap: bad argument"),
    ("gs_frame_ingest", dict(n_out=3), EINVAL, "gs_frame_ingest: n_out must be 1 or 2"),
    ("gs_frame_ingest", dict(image=None), EINVAL, "gs_frame_ingest: null pointer"),
    ("gs_frame_ingest", dict(n_out=2, depth1=None), EINVAL, "gs_frame_ingest: null pointer"),
    ("gs_frame_ingest", dict(width=0), EINVAL, "gs_frame_ingest: source size out of range (1 <= width, height <= 16384)"),
    ("gs_frame_ingest", dict(h_sizes=lambda: (C.c_int32 * 4)(1, 16385, 1, 1)), EINVAL,
     "gs_frame_ingest: output size out of range (1 <= W, H <= 16384)"),
    # completion / accuracy judge, evaluation
    ("gs_depth_cloud", dict(height=0), EINVAL, "gs_depth_cloud: image size out of range (1 <= width, height <= 16384)"),
    ("gs_depth_cloud", dict(valid=None), EINVAL, "gs_depth_cloud: null pointer"),
    ("gs_depth_cloud", dict(h_intrinsics4=lambda: (C.c_float * 4)(1, 0, 0, 0)), EINVAL, "gs_depth_cloud: fx and fy must not be zero"),
    ("gs_depth_cloud", dict(h_intrinsics4=lambda: (C.c_float * 4)(math.nan, 1, 0, 0)), EINVAL, "gs_depth_cloud: fx and fy must not be zero"),
    ("gs_cloud_nearest", dict(n_query=-1), EINVAL, "gs_cloud_nearest: size out of range (0 <= n_query, n_points <= 2^30)"),
    ("gs_cloud_nearest", dict(flags=4), EINVAL, "gs_cloud_nearest: unknown flag"),
    ("gs_cloud_nearest", dict(out=None), EINVAL,
     "gs_cloud_nearest: null pointer (only query_valid and points_valid may be null) or scratch not 4-byte aligned"),
    ("gs_cloud_nearest", dict(scratch=BUF + 2), EINVAL,
     "gs_cloud_nearest: null pointer (only query_valid and points_valid may be null) or scratch not 4-byte aligned"),
    ("gs_completion_row", dict(n_samples=0), EINVAL, "gs_completion_row: size out of range (1 <= n_samples <= 2^30, 0 <= n_acc <= 2^30)"),
    ("gs_completion_row", dict(row6=BUF + 4), EINVAL,
     "gs_completion_row: null pointer (only acc_valid may be null), or scratch / row6 not 8-byte aligned"),
    ("gs_eval_frame_layout", dict(layout=None), EINVAL, "gs_eval_frame_layout: null pointer"),
    ("gs_eval_frame_layout", dict(width=0), EINVAL, "gs_eval_frame_layout: image size out of range (1 <= width, height <= 16384)"),
    ("gs_eval_frame_layout", dict(flags=16), EINVAL, "gs_eval_frame_layout: unknown flag"),
    ("gs_eval_frame", dict(height=16385), EINVAL, "gs_eval_frame: image size out of range (1 <= width, height <= 16384)"),
    ("gs_eval_frame", dict(flags=16), EINVAL, "gs_eval_frame: unknown flag"),
    ("gs_eval_frame", dict(width=160, height=200, flags=8), EINVAL,
     "gs_eval_frame: GS_EVAL_MS_SSIM needs min(width, height) > 160 (five scales of an 11-tap valid window)"),
    ("gs_eval_frame", dict(gt_im=None), EINVAL, "gs_eval_frame: null pointer, or scratch / row not 8-byte aligned"),
    ("gs_eval_frame", dict(row=BUF + 4), EINVAL, "gs_eval_frame: null pointer, or scratch / row not 8-byte aligned"),
]


def _parameter_names():
    """entry point -> its parameter names, in the order of the prototype in include/gsplat_hip.h"""
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(gs_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src):
        params = " ".join(params.split())
        out[name] = [] if params in ("", "void") else [re.findall(r"\w+", p)[-1] for p in params.split(",")]
    return out


def _value(v):
    return v() if callable(v) else v


def _arguments(lib, names, entry, given):
    fn = getattr(lib, entry)
    assert len(fn.argtypes) == len(names[entry]), entry
    assert set(given) <= set(names[entry]), (entry, set(given) - set(names[entry]))
    keep, args = [], []
    for name, t in zip(names[entry], fn.argtypes):
        if name in given:
            v = _value(given[name])
        elif name in PLAUSIBLE.get(entry, {}):
            v = _value(PLAUSIBLE[entry][name])
        elif name == "cam":
            v = cam()
        elif name == "stream":
            v = None
        elif t is C.c_void_p:
            v = BUF
        elif hasattr(t, "contents"):                   # a typed pointer
            v = C.cast(BUF, t)
        elif t in (C.c_float, C.c_double):
            v = 1.0
        else:
            v = 0 if name in ZERO_BY_DEFAULT else 1
        if v is not None and not isinstance(v, (int, float)):
            keep.append(v)                             # (host arrays stay alive over the call)
            if t is C.c_void_p:
                v = C.cast(v, C.c_void_p)
        args.append(v)
    return args, keep


def _check_table(lib):
    names = _parameter_names()
    wrong = []
    for entry, given, code, text in REFUSALS:
        args, keep = _arguments(lib, names, entry, given)
        rc = getattr(lib, entry)(*args)
        got = lib.gs_last_error().decode()
        if rc != code or got != text:
            wrong.append((entry, given, rc, got))
    assert not wrong, wrong


def test_every_refusal_of_the_hip_library():
    import __graft_entry__ as ge
    from activesplat_amd import _lib
    ge.build()
    _lib.unload_for_tests()
    _check_table(_lib.get())


def test_every_refusal_of_the_emulated_build(emu_lib_path):
    from activesplat_amd import _lib
    try:
        _check_table(_lib.load_for_tests(emu_lib_path))
    finally:
        _lib.unload_for_tests()

