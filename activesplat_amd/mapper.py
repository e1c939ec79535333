"""Mapping-loop harness: this build's counterpart of the reference's `SplaTAM.__mapping`
(src/mapper/splatam/__init__.py:254-542), which cannot be imported or shipped (it pulls in cv2, open3d, rospy,
habitat).  It reproduces the CALL PATTERN and SCHEDULE of the hot loop, nothing of the ROS/GUI shell:

  frame 0                       : back-project the RGB-D frame -> initialize_params; scene_radius = max depth / 3
                                  (__init__.py:382-386, config/splatam/online_habitat_sim.py:6)
  every frame                   : write the ground-truth pose into params['cam_*'][..., id] (tracking is skipped,
                                  __init__.py:400-405) -- or, with tracking=dict(use_gt_poses=False), frame 0 takes its pose and
                                  every later frame is TRACKED (mapping.initialize_camera_pose + mapping.track_frame, SplaTAM's
                                  loop) before the high-loss render, growth and mapping, which all use the tracked pose
  frames with id == 0 or (id+1) % map_every == 0
                                : add_new_gaussians (id > 0), keyframe_selection_overlap over keyframe_list[:-1]
                                  (window = mapping_window_size - 2, + last keyframe + current frame), FRESH Adam
                                  (__init__.py:408-440)
  iterations                    : iter_per_frame = mapping_iters // map_every, or mapping_iters when that is 0 and
                                  id % map_every == 0 (__init__.py:395-397); each: np.random.randint keyframe pick,
                                  get_loss (two raster passes), backward, optional prune / densify, Adam step,
                                  zero_grad(set_to_none) (__init__.py:447-480)
  keyframes                     : appended when id == 0, (id+1) % keyframe_every == 0 or id == step_num - 2, unless the
                                  frame's ground-truth pose holds inf / nan (__init__.py:514-524)
  every frame once a map exists : get_high_loss_samples' render of the map at the frame's pose (two raster passes in the
                                  reference, one with fused_render) and its "rendered surface in front of a measured one" mask
                                  (__init__.py:184-214, 256-258).  With high_loss_target=True the rest of that method runs on the
                                  device too (visibility.high_loss_grid: the mask and its resize to one pixel per degree in one
                                  launch; visibility.grid_dbscan), and `high_loss_samples_pose_c2w` resolves the look target
                                  (__init__.py:216-250) from one small copy when it is first read
  frame 0 and frames with (id+1) % report_global_progress_every == 0, when they ran iterations, `report_progress` on
                                : report_progress(mapping=True) of the frame (__init__.py:499-505): PSNR, "Depth RMSE", depth L1 -- one render and
                                  one library call into the table `progress` (evaluate.MapEvaluator; rows are read when the caller asks for them)
  every frame, `judge` set      : the completion / accuracy judge of scripts/judges/eval_actions.py on the frame's sensor depth at its
                                  ground-truth pose (judge.CompletionJudge.add_frame; rows are read when the caller asks for them)

Inputs are already-resized frames (`color [3,H,W]` in 0..1, `depth [1,H,W]` metres, pose relative to frame 0 as
quaternion (w,x,y,z) + translation of the w2c) -- the cv2 resize / PNG / manifest work of the reference is I/O
outside the hot path.  Defaults are the shipped configuration (config/splatam/online_habitat_sim.py,
config/datasets/gibson.json).
"""
from __future__ import annotations

import copy
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import mapping as M
from . import optim as O
from .camera import setup_camera
from . import frames as FR
from .keyframes import keyframe_selection_overlap

DEFAULT_CONFIG = dict(
    seed=0, gaussian_distribution="anisotropic", scene_radius_depth_ratio=3, mean_sq_dist_method="projective",
    map_every=5, keyframe_every=5, mapping_window_size=12, mapping_iters=2, step_num=1000,
    # False = the reference's call pattern; True = the fused HIP paths of this build (same loss, see mapping.get_loss)
    fused_render=False,      # one raster pass per iteration (rasterizer.render_rgbd) instead of two
    fused_loss=False,        # masked-L1 + L1 + SSIM value and gradients by gs_mapping_loss
    fused_inputs=False,      # transform_to_frame + activations by gs_activate_*
    fused_preprocess=False,  # ... or inside the rasteriser's per-Gaussian kernels (rasterizer.render_rgbd_raw; needs fused_render): no activation launches
    fused_adam=False,        # ... and the Adam step of an iteration inside that render's backward kernel (needs fused_preprocess; iterations whose
                             # prune / densify event replaces the parameter tensors take the separate step, as the reference's loop effectively does)
    fused_iteration=False,   # ... and the whole iteration (get_loss + backward + step + zero_grad) as four library calls without autograd
                             # (mapping.mapping_iteration; needs fused_render, fused_loss, fused_preprocess; event iterations take the usual path)
    fused_growth=False,      # add_new_gaussians: one forward + gs_grow_gaussians
    fused_tracking=False,    # tracking (tracking.use_gt_poses=False): mapping.track_frame's HIP loop (tracking_iteration) instead of the reference pattern
    device_ingest=False,     # run_raw: the raw frame goes up once through pinned buffers and gs_frame_ingest writes both resolutions (ingest.FrameIngest)
                             # instead of two host resizes and pageable copies; the frame's pose floats travel with it and the keyframe decision is
                             # made on the host pose.  The same frame tensors, bit for bit; a frame whose image is not uint8 takes the host path
    fused_keyframes=True,    # (accepted for older configs; no effect: the keyframe overlap scores always come from gs_keyframe_overlap, one launch)
    high_loss_samples=True,  # the per-frame no-grad render of get_high_loss_samples (__init__.py:184-258) before mapping a frame
    high_loss_target=False,  # ... and the rest of get_high_loss_samples on the device (gs_high_loss_grid + gs_grid_dbscan): the look target of the
                             # frame is then `SplatMapper.high_loss_samples_pose_c2w`, resolved from one small copy when it is read
    report_progress=False,   # report_progress(mapping=True) after the iterations of frame 0 and of every report_global_progress_every-th frame
                             # (eval_helpers.py:153-264): one row of `SplatMapper.progress` per reported frame.  Off: run() issues what it issued without the key
    report_global_progress_every=100,
    cluster_invisibility_threshold=25,   # config/datasets/gibson.json:60
    high_loss_fov=(90, 90),  # (hfov, vfov) of get_high_loss_samples: the grid has one pixel per degree
    mapping=dict(
        loss_weights=dict(im=0.5, depth=1.0), sil_thres=0.98, use_sil_for_loss=False, use_l1=True,
        ignore_outlier_depth_loss=False, add_new_gaussians=True, prune_gaussians=False,
        use_gaussian_splatting_densification=False,
        lrs=dict(means3D=0.0001, rgb_colors=0.0025, unnorm_rotations=0.001, logit_opacities=0.05, log_scales=0.001,
                 cam_unnorm_rots=0.0, cam_trans=0.0),
        pruning_dict=dict(start_after=0, remove_big_after=0, stop_after=20, prune_every=20, removal_opacity_threshold=0.005,
                          final_removal_opacity_threshold=0.005, reset_opacities=False, reset_opacities_every=500),
        densify_dict=dict(start_after=500, remove_big_after=3000, stop_after=5000, densify_every=100, grad_thresh=0.0002,
                          num_to_split_into=2, removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005,
                          reset_opacities=False, reset_opacities_every=3000)),
    # the reference's tracking section (config/splatam/online_habitat_sim.py:20-45, mapping.TRACKING_DEFAULTS) -- except use_gt_poses, True
    # here: the reference mapper writes the simulator's poses whatever its config says (__init__.py:400-405), and so does this one by default
    tracking=dict(M.TRACKING_DEFAULTS, use_gt_poses=True),
    viz=dict(viz_near=0.01, viz_far=100.0),
)


class SplatMapper:
    def __init__(self, intrinsics, width, height, config=None, device=None):
        self.cfg = copy.deepcopy(DEFAULT_CONFIG)
        if config:
            for k, v in config.items():
                if isinstance(v, dict) and isinstance(self.cfg.get(k), dict):
                    self.cfg[k].update(v)
                else:
                    self.cfg[k] = v
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.W, self.H = int(width), int(height)
        self.intrinsics = torch.as_tensor(np.asarray(intrinsics), dtype=torch.float32, device=self.device)
        self._k_host = np.asarray(intrinsics, dtype=np.float64)
        self._pose_host = {}               # frame id -> (quaternion, translation) as this mapper wrote them into the camera parameters (host tensors)
        lrs = self.cfg["mapping"]["lrs"]
        self.cfg["tracking"] = M.tracking_config(self.cfg["tracking"])
        self._tracking = not self.cfg["tracking"]["use_gt_poses"]
        self._poses_fixed = float(lrs.get("cam_unnorm_rots", 0.0)) == 0.0 and float(lrs.get("cam_trans", 0.0)) == 0.0 and not self._tracking
        self.first_frame_w2c = torch.eye(4, device=self.device)
        self.cam = setup_camera(self.W, self.H, np.asarray(intrinsics), np.eye(4), device=self.device)
        self.densify_cam, self.densify_intrinsics = self.cam, self.intrinsics      # replaced when frames carry a densify copy
        self.first_abs_pose = None
        self._one = M.unit_gradient(torch.empty((), dtype=torch.float32, device=self.device))   # (the fused loss knows it: no scaling launch)
        self.params = self.variables = self.optimizer = None
        self.keyframe_list, self.selected_keyframes, self.gt_w2c_all_frames = [], [], []
        self.rng = np.random.RandomState(self.cfg["seed"])
        self.stats = dict(iters=0, iter_time=0.0, frames=0, frame_time=0.0, tracking_iters=0, tracking_time=0.0, tracked_frames=0)
        self._last_losses = None           # device scalars of the most recent iteration (read through `last_losses`)
        self.high_loss_mask = None          # bool [H,W] of the most recent frame (None before the first map exists)
        self.high_loss_grid = None          # float32 [vfov, hfov] of 0 / 1 (high_loss_target=True): the reference's non_presence_depth_mask_cv2 / 255
        self._high_loss_pending = None      # (host w2c or None, device w2c or None, GridClusters) of the most recent frame, until the pose is read
        self._high_loss_pose = None
        #: a judge.CompletionJudge, or None (the default: nothing changes).  When set, run() hands every frame's sensor depth, the inverse of
        #: the frame's INPUT pose (the ground-truth pose also when tracking is on: this is what the reference's judge replays) and
        #: frame.get("path_length", 0.0) to judge.add_frame -- three library calls, no host wait.  The poses are relative to frame 0's
        #: camera, so the judge's samples must be given in that frame; transforming a mesh into it is the caller's work.
        self.judge = None
        #: evaluate.MapEvaluator of the reported frames (config report_progress; None until the first report) and their frame ids
        self.progress = None
        self.progress_frames = []
        self._ingest = None                 # ingest.FrameIngest of the current source size (device_ingest=True; built on first use)

    @property
    def last_losses(self):
        """{name: float} of the most recent mapping iteration (None before the first); synchronises with the device."""
        if self._last_losses is None:
            return None
        return {k: float(v.detach()) for k, v in self._last_losses.items()}

    @property
    def high_loss_samples_pose_c2w(self):
        """The look target of the most recent frame (get_high_loss_samples' return value; needs high_loss_target=True): the frame's camera turned
        towards the centre of the largest high-loss cluster, or None -- also before the first map exists.  run() only enqueues the kernels; the first
        read makes ONE small device-to-host copy (the grid's sum, the cluster table and, for a tracked frame, the pose matrix), which synchronises
        with the device, and the result is kept for that frame."""
        if self._high_loss_pending is not None:
            from . import visibility as VIS
            w2c_host, w2c_dev, g = self._high_loss_pending
            hfov, vfov = (int(v) for v in self.cfg["high_loss_fov"])
            tensors = [g.total.reshape(1), g.n_clusters.reshape(1), g.count, g.sum_row, g.sum_col] + ([w2c_dev] if w2c_dev is not None else [])
            tot, n, count, sr, sc, *pose = VIS._one_copy(tensors)
            total, m = float(tot[0]), int(n[0])
            if m > count.shape[0]:                       # (more clusters than rows in the table: once more with enough rows)
                total, count, sr, sc, _ = VIS.high_loss_clusters(self.high_loss_grid, m)
            w2c = pose[0] if pose else w2c_host.numpy()
            self._high_loss_pose = VIS.target_from_high_loss_clusters(np.linalg.inv(w2c.astype(np.float64)), total, count[:m], sr[:m], sc[:m],
                                                                      self.cfg["cluster_invisibility_threshold"], hfov, vfov)
            self._high_loss_pending = None
        return self._high_loss_pose

    # -- helpers ---------------------------------------------------------------------------------
    @staticmethod
    def _w2c_host(quat, pos):
        """4x4 w2c of a (w,x,y,z) quaternion + translation, on the HOST (the same torch ops as on the device, ~15 of them: issued as
        device launches they were 0.3 ms of host time per call, several times per frame)."""
        w2c = torch.eye(4)
        w2c[:3, :3] = M.build_rotation(F.normalize(quat.view(1, 4)))
        w2c[:3, 3] = pos
        return w2c

    def _w2c(self, frame_id):
        # the poses this mapper wrote into the camera parameters are still on the host (tracking is skipped and their learning rates are
        # zero in the shipped configuration); a pose that is optimised is read from the parameters
        host = self._pose_host.get(int(frame_id)) if self._poses_fixed else None
        if host is not None:
            return self._w2c_host(*host).to(self.device)
        rot = F.normalize(self.params["cam_unnorm_rots"][..., frame_id].detach())
        w2c = torch.eye(4, device=self.device)
        w2c[:3, :3] = M.build_rotation(rot)
        w2c[:3, 3] = self.params["cam_trans"][..., frame_id].detach()
        return w2c

    def _data(self, color, depth, frame_id):
        return {"cam": self.cam, "im": color, "depth": depth, "id": frame_id, "intrinsics": self.intrinsics,
                "w2c": self.first_frame_w2c}

    # -- one frame of the mapper (reference: SplaTAM.__mapping) ----------------------------------------
    def run(self, frame):
        cfg, mc = self.cfg, self.cfg["mapping"]
        fid = int(frame["id"])
        color = frame["color"].to(self.device).float()
        depth = frame["depth"].to(self.device).float()
        quat_h = torch.as_tensor(np.asarray(frame["quat"], dtype=np.float32)).reshape(4).clone()
        pos_h = torch.as_tensor(np.asarray(frame["position"], dtype=np.float32)).reshape(3).clone()
        self._pose_host[fid] = (quat_h, pos_h)
        if "quat_device" in frame and "position_device" in frame:      # (run_raw with device_ingest: already uploaded with the frame)
            quat, pos = frame["quat_device"], frame["position_device"]
        else:
            quat, pos = quat_h.to(self.device), pos_h.to(self.device)
        if self.judge is not None:
            c2w = np.linalg.inv(self._w2c_host(quat_h, pos_h).numpy().astype(np.float64))
            self.judge.add_frame(depth.reshape(depth.shape[-2], depth.shape[-1]).contiguous(), self._k_host, c2w, float(frame.get("path_length", 0.0)))
        tracked = self._tracking and fid > 0 and self.params is not None
        if tracked:
            # SplaTAM's tracking of this frame: constant-velocity start, then the tracking loop; the frame's own pose only goes to gt_w2c_all_frames
            t_track = time.perf_counter()
            M.initialize_camera_pose(self.params, fid, self.cfg["tracking"]["forward_prop"])
            res = M.track_frame(self.params, self._data(color, depth, fid), self.variables, fid, self.cfg["tracking"],
                                fused=cfg.get("fused_tracking", False))
            self.stats["tracking_iters"] += res["iterations"]
            self.stats["tracking_time"] += time.perf_counter() - t_track
            self.stats["tracked_frames"] += 1
        self._high_loss_pending = self._high_loss_pose = None
        if self.params is not None and (cfg.get("high_loss_samples", True) or cfg.get("high_loss_target", False)):
            view = self._w2c(fid) if tracked else self._w2c_host(quat_h, pos_h)      # (host pose: the camera block is built on the host)
            self.high_loss_step(view, depth, tracked)
        # densification-resolution copy of the frame (reference :362-376); defaults to the mapping resolution
        d_color = frame["densify_color"].to(self.device).float() if "densify_color" in frame else color
        d_depth = frame["densify_depth"].to(self.device).float() if "densify_depth" in frame else depth
        if fid == 0 and d_color.shape[1:] != color.shape[1:]:
            fac = color.shape[2] / d_color.shape[2]
            self.densify_intrinsics = FR.densify_intrinsics(self.intrinsics.cpu(), fac).to(self.device)
            self.densify_cam = setup_camera(d_color.shape[2], d_color.shape[1], self.densify_intrinsics.cpu().numpy(), np.eye(4),
                                            device=self.device)
        if fid == 0:
            init_w2c = torch.eye(4)
            init_w2c[:3, :3] = M.build_rotation(quat_h.view(1, 4))
            init_w2c[:3, 3] = pos_h
            init_w2c = init_w2c.to(self.device)
            mask = (d_depth > 0).reshape(-1)
            cld, msd = M.get_pointcloud(d_color, d_depth, self.densify_intrinsics, init_w2c, mask=mask, compute_mean_sq_dist=True)
            self.params, self.variables = M.initialize_params(cld, cfg["step_num"], msd, cfg["gaussian_distribution"])
            self.variables["scene_radius"] = torch.max(d_depth) / cfg["scene_radius_depth_ratio"]
        map_every = cfg["map_every"]
        iter_per_frame = int(cfg["mapping_iters"] // map_every)
        if iter_per_frame == 0 and fid % map_every == 0:
            iter_per_frame = cfg["mapping_iters"]
        if not tracked:
            with torch.no_grad():                                # tracking skip: ground-truth pose (and frame 0's pose when tracking)
                self.params["cam_unnorm_rots"][..., fid] = quat
                self.params["cam_trans"][..., fid] = pos
        if fid == 0 or (fid + 1) % map_every == 0:
            if mc["add_new_gaussians"] and fid > 0:
                d_data = {"cam": self.densify_cam, "im": d_color, "depth": d_depth, "id": fid, "intrinsics": self.densify_intrinsics,
                          "w2c": self.first_frame_w2c}
                pose7 = None
                if cfg.get("fused_growth", False):
                    q_g, t_g = (self.params["cam_unnorm_rots"][0, :, fid].detach().cpu(), self.params["cam_trans"][0, :, fid].detach().cpu()) \
                        if tracked else (quat_h, pos_h)
                    pose7 = [float(v) for v in F.normalize(q_g.view(1, 4)).view(4).tolist()] + [float(v) for v in t_g.tolist()]
                self.params, self.variables = M.add_new_gaussians(self.params, self.variables, d_data,
                                                                  mc["sil_thres"], fid, cfg["gaussian_distribution"],
                                                                  fused=cfg.get("fused_growth", False), pose7=pose7)
            with torch.no_grad():
                sel = keyframe_selection_overlap(depth, self._w2c(fid), self.intrinsics, self.keyframe_list[:-1],
                                                 cfg["mapping_window_size"] - 2)
                self.selected_keyframes = [int(s) for s in sel]
                if len(self.keyframe_list) > 0:
                    self.selected_keyframes.append(len(self.keyframe_list) - 1)
                self.selected_keyframes.append(-1)
            self.optimizer = O.initialize_optimizer(self.params, mc["lrs"], tracking=False)
        t_frame = time.perf_counter()
        for it in range(iter_per_frame):
            t0 = time.perf_counter()
            pick = self.selected_keyframes[self.rng.randint(0, len(self.selected_keyframes))]
            if pick == -1:
                it_id, it_color, it_depth = fid, color, depth
            else:
                kf = self.keyframe_list[pick]
                it_id, it_color, it_depth = kf["id"], kf["color"], kf["depth"]
            # ONE predicate for both fused forms: does this iteration's prune / densify call move rows or reset parameters (then the tensors are
            # replaced between backward and step, and the separate step is taken, as the reference's loop effectively does)?
            event = (mc["prune_gaussians"] and O.prune_event(it, mc["pruning_dict"])) \
                or (mc["use_gaussian_splatting_densification"] and O.densify_event(it, mc["densify_dict"]))
            fused_path = cfg.get("fused_preprocess", False) and cfg["fused_render"] and not event
            in_backward = cfg.get("fused_adam", False) and fused_path
            # (fused_iteration IS the Adam-inside-the-backward form without autograd: it implies fused_adam whatever the config says)
            direct = cfg.get("fused_iteration", False) and fused_path and cfg["fused_loss"] and mc["use_l1"]
            if direct:
                # the whole iteration without autograd.  No event here, so prune_gaussians is a no-op by its own predicate (prune_event) and
                # densify only accumulates this iteration's statistics; nothing holds a gradient afterwards, so step() / zero_grad() have
                # nothing to do -- asserted, so that a parameter that starts receiving gradients (camera learning rates > 0) cannot be skipped
                loss, self.variables, losses = M.mapping_iteration(self.params, self._data(it_color, it_depth, it_id), self.variables, it_id,
                                                                   mc["loss_weights"], self.optimizer,
                                                                   ignore_outlier_depth_loss=mc["ignore_outlier_depth_loss"])
                if mc["use_gaussian_splatting_densification"]:
                    self.params, self.variables = O.densify(self.params, self.variables, self.optimizer, it, mc["densify_dict"])
                if any(p.grad is not None for p in self.params.values()):
                    raise RuntimeError("SplatMapper(fused_iteration=True): a parameter holds a gradient after the autograd-free iteration -- "
                                       "this loop would never step it; use fused_iteration=False")
                self._last_losses = {k: v.detach() for k, v in losses.items()}
                self.stats["iters"] += 1
                self.stats["iter_time"] += time.perf_counter() - t0
                continue
            loss, self.variables, losses = M.get_loss(self.params, self._data(it_color, it_depth, it_id), self.variables, it_id,
                                                      mc["loss_weights"], mc["use_sil_for_loss"], mc["sil_thres"], mc["use_l1"],
                                                      mc["ignore_outlier_depth_loss"], fused=cfg["fused_render"], fused_loss=cfg["fused_loss"],
                                                      fused_inputs=cfg["fused_inputs"], fused_preprocess=cfg.get("fused_preprocess", False),
                                                      fused_adam=self.optimizer if in_backward else None)
            with M.backward_on_calling_thread():        # (no hand-over to autograd's device thread: mapping.backward_on_calling_thread)
                loss.backward(gradient=self._one)       # cached dL/dloss = 1: saves autograd's ones_like launch per iteration
            with torch.no_grad():
                if mc["prune_gaussians"]:
                    self.params, self.variables = O.prune_gaussians(self.params, self.variables, self.optimizer, it, mc["pruning_dict"])
                if mc["use_gaussian_splatting_densification"]:
                    self.params, self.variables = O.densify(self.params, self.variables, self.optimizer, it, mc["densify_dict"])
                self.optimizer.step()
                self.optimizer.zero_grad(set_to_none=True)
            self._last_losses = {k: v.detach() for k, v in losses.items()}   # (no graph kept alive) converted on access: a float() here would stall the host every iteration
            self.stats["iters"] += 1
            self.stats["iter_time"] += time.perf_counter() - t0
        if iter_per_frame > 0:
            self.stats["frames"] += 1
            self.stats["frame_time"] += time.perf_counter() - t_frame
            if cfg.get("report_progress", False) and (fid == 0 or (fid + 1) % int(cfg["report_global_progress_every"]) == 0):
                self.report_progress(fid, color, depth)
        with torch.no_grad():
            # the simulator's pose when the caller hands one over (run_raw), the pose written into the camera parameters otherwise
            # (tracking: the frame's own pose -- the parameters hold the estimate)
            pose_ok = None
            if cfg.get("device_ingest", False) and ("gt_w2c" in frame or self._tracking or self._poses_fixed):
                # the pose is known on the host: the same decision from the host values, without reading the device
                gt_host = torch.as_tensor(np.asarray(frame["gt_w2c"]), dtype=torch.float32) if "gt_w2c" in frame else self._w2c_host(quat_h, pos_h)
                pose_ok = bool(torch.isfinite(gt_host).all())
                gt_w2c = frame["gt_w2c_device"].clone() if "gt_w2c_device" in frame else gt_host.to(self.device)
            else:
                gt_w2c = torch.as_tensor(np.asarray(frame["gt_w2c"]), dtype=torch.float32, device=self.device) if "gt_w2c" in frame \
                    else (self._w2c_host(quat_h, pos_h).to(self.device) if self._tracking else self._w2c(fid))
            if pose_ok is None:
                pose_ok = bool(torch.isfinite(gt_w2c).all())
            if (fid == 0 or (fid + 1) % cfg["keyframe_every"] == 0 or fid == cfg["step_num"] - 2) and pose_ok:
                self.keyframe_list.append({"id": fid, "est_w2c": self._w2c(fid), "color": color, "depth": depth})
            self.gt_w2c_all_frames.append(gt_w2c)
        return self.params

    @torch.no_grad()
    def report_progress(self, fid, color, depth):
        """report_progress(mapping=True) of frame `fid` (eval_helpers.py:211-245: no silhouette mask, images not masked by the depth): one fused render
        at the frame's pose column and one gs_eval_frame into `progress`.  Only enqueues work."""
        from . import evaluate as E
        if self.progress is None:
            every = max(1, int(self.cfg["report_global_progress_every"]))
            self.progress = E.MapEvaluator(self.W, self.H, int(self.cfg["step_num"]) // every + 2, device=self.device)
        host = self._pose_host.get(int(fid)) if self._poses_fixed else None      # (an optimised pose is read from the parameters: one small copy)
        pose7 = None if host is None else [float(v) for v in F.normalize(host[0].view(1, 4)).view(4).tolist()] + [float(v) for v in host[1].tolist()]
        im, rdepth, sil = E.render_frame(self.params, self.cam, fid, pose7)
        self.progress.add_frame(im.contiguous(), rdepth.contiguous(), sil.contiguous(), color.contiguous(), depth.contiguous(),
                                self.cfg["mapping"]["sil_thres"], sil_mask=False, image_valid_mask=False, ssim=False, ms_ssim=False)
        self.progress_frames.append(int(fid))

    def evaluate(self, frames, eval_every=1, ssim=True, ms_ssim=True):
        """The reference's end-of-run `eval` of this mapper's map over `frames` (evaluate.evaluate_map) -> its dict."""
        from . import evaluate as E
        mc = self.cfg["mapping"]
        return E.evaluate_map(self.params, frames, self._k_host, self.first_frame_w2c, mc["sil_thres"], self.cfg["mapping_iters"],
                              mc["add_new_gaussians"], eval_every=eval_every, ssim=ssim, ms_ssim=ms_ssim)

    @torch.no_grad()
    def high_loss_step(self, view_w2c, gt_depth, tracked=False):
        """The per-frame step of run(): `high_loss_mask` of the frame and, with high_loss_target=True, `high_loss_grid` and the clustering that
        `high_loss_samples_pose_c2w` resolves when it is read (tracked: view_w2c is the tracker's pose, a device tensor that travels in that copy).  Only
        enqueues work: the render, then -- for the target -- two library calls in place of the mask's torch expression."""
        self._high_loss_pending = self._high_loss_pose = None
        if not self.cfg.get("high_loss_target", False):
            self.high_loss_mask = self.high_loss_samples_mask(view_w2c, gt_depth)
            return
        from . import visibility as VIS
        _, depth, opacity = self.render_rgbd(view_w2c)
        hfov, vfov = (int(v) for v in self.cfg["high_loss_fov"])
        self.high_loss_mask, self.high_loss_grid = VIS.high_loss_grid(depth, opacity, gt_depth, hfov, vfov)
        g = VIS.grid_dbscan(self.high_loss_grid, 0.0, VIS.HIGH_LOSS_EPS, VIS.HIGH_LOSS_MIN_SAMPLES)
        self._high_loss_pending = (None, view_w2c, g) if tracked else (view_w2c, None, g)

    @torch.no_grad()
    def high_loss_samples_mask(self, view_w2c, gt_depth):
        """The render + mask half of get_high_loss_samples (__init__.py:184-214): the map rendered at the frame's pose, and
        `rendered depth > measured depth  and  |error| > 0.3 m (measured pixels only)  and  opacity > 0.8` -- regions where the map
        shows a surface in front of free space the sensor saw through.  Stays on the device; the caller's clustering is not ours."""
        im, depth, opacity = self.render_rgbd(view_w2c)
        gt = gt_depth if gt_depth.dim() == 3 else gt_depth.unsqueeze(0)
        err = (depth - gt).abs() * (gt > 0)
        return ((depth > gt) & (err > 0.3) & (opacity > 0.8))[0]

    def run_raw(self, image, depth, X_WV, frame_id, quat, position):
        """Sensor frame in (uint8 [h,w,3] image, [h,w] metric depth, 4x4 pose X_WV): pre-processing of :332-378 (pose to the
        relative OpenGL-convention w2c, resize to the mapping resolution and to the densification resolution), then run().
        quat (w,x,y,z) / position are the tracker's camera parameters for this frame (the reference skips tracking and
        writes the simulator's, :400-405)."""
        gt_w2c, self.first_abs_pose = FR.gt_w2c_from_pose(X_WV, self.first_abs_pose)
        if self.cfg.get("device_ingest", False) and getattr(image, "dtype", None) in (np.uint8, torch.uint8):
            return self.run(self._ingest_raw(image, depth, gt_w2c, frame_id, quat, position))
        color, d = FR.to_mapping_tensors(image, depth, self.W, self.H, self.device)
        fac = float(self.cfg.get("densify_downscale_factor", 1))
        frame = {"id": frame_id, "color": color, "depth": d, "quat": quat, "position": position, "gt_w2c": gt_w2c}
        if fac != 1:
            frame["densify_color"], frame["densify_depth"] = FR.to_mapping_tensors(image, depth, int(self.W / fac), int(self.H / fac),
                                                                                   self.device)
        return self.run(frame)

    def run_sensor(self, sensor, X_WV, frame_id, quat, position):
        """run_raw with the frame produced on the device: `sensor` (sensor.MeshSensor) renders the mesh at the pose X_WV -- the pose run_raw
        takes --, gs_frame_ingest resizes its device tensors to the mapping and the densification resolution, then run().  No pixel goes to
        the host; the sensor's two tile-list counters do (sensor.render_mesh).  The frame is on the device already, so this ALWAYS takes the
        device ingest (ingest.FrameIngest, the pose through its pinned slot), whatever cfg["device_ingest"] says: that key chooses run_raw's path only."""
        image, depth = sensor.frame(X_WV)
        gt_w2c, self.first_abs_pose = FR.gt_w2c_from_pose(X_WV, self.first_abs_pose)
        return self.run(self._ingest_raw(image, depth, gt_w2c, frame_id, quat, position))

    def _ingest_raw(self, image, depth, gt_w2c, frame_id, quat, position):
        """run_raw's frame dict with device_ingest: one upload and one launch for both resolutions (ingest.FrameIngest)."""
        from . import ingest as IN
        h, w = int(image.shape[0]), int(image.shape[1])
        fac = float(self.cfg.get("densify_downscale_factor", 1))
        sizes = [(self.W, self.H)] + ([(int(self.W / fac), int(self.H / fac))] if fac != 1 else [])
        if self._ingest is None or (self._ingest.w, self._ingest.h) != (w, h) or self._ingest.sizes != sizes:
            self._ingest = IN.FrameIngest(w, h, sizes, self.device)
        outs, quat_d, pos_d, gt_d = self._ingest.put(image, depth, quat, position, gt_w2c)
        frame = {"id": frame_id, "color": outs[0][0], "depth": outs[0][1], "quat": quat, "position": position, "gt_w2c": gt_w2c,
                 "quat_device": quat_d, "position_device": pos_d, "gt_w2c_device": gt_d}
        if len(outs) == 2:
            frame["densify_color"], frame["densify_depth"] = outs[1]
        return frame

    # -- hand-off (reference: q_main2vis.put(GaussianPacket(...)) __init__.py:536-542; post_processing :544-578) ----
    def packet(self, c2w=None):
        from .io import GaussianPacket
        return GaussianPacket(self.params, c2w)

    def post_processing(self, output_dir):
        """Writes params.npz with the reference's 14 keys (cam_* trimmed to the mapped frames)."""
        from . import io as IO
        kf_ids = [int(k["id"]) for k in self.keyframe_list]
        out = IO.finalize_params(self.params, self.variables, self.intrinsics, self.first_frame_w2c, self.W, self.H,
                                 self.gt_w2c_all_frames, kf_ids)
        return IO.save_params(out, output_dir)

    @torch.no_grad()
    def look_around(self, view_c2w, scale_modifier=1.0, fused=True):
        """360-degree opacity / RGB / depth panorama of the planner (lookaround.py)."""
        from . import lookaround as LA
        return LA.look_around(self.params, view_c2w, scale_modifier, fused)

    @torch.no_grad()
    def global_invisibility_nodes(self, view_c2w, positions, scale_modifier=1.0, max_clusters=256, nodes_per_pass=None):
        """Per Voronoi node of `positions` [K, 3]: the panorama's depth, invisibility, DBSCAN labels and cluster table -- what
        get_convexhull_volume holds after its DBSCAN line -- with one device-to-host copy for all nodes (visibility.py)."""
        from . import visibility as VIS
        return VIS.global_invisibility_nodes(self.params, view_c2w, positions, scale_modifier, max_clusters, nodes_per_pass)

    @torch.no_grad()
    def global_invisibility_scores(self, view_c2w, positions, scale_modifier=1.0, max_clusters=256, nodes_per_pass=None):
        """Per Voronoi node of `positions` [K, 3] the two floats of get_global_invisibility, (invisibility [K], volume [K]) float64 -- renders,
        DBSCAN, contours and hull volumes on the device, one small copy (visibility.py)."""
        from . import visibility as VIS
        return VIS.global_invisibility_scores(self.params, view_c2w, positions, scale_modifier, max_clusters, nodes_per_pass)

    @torch.no_grad()
    def local_invisibility_target(self, view_c2w, cluster_invisibility_threshold=30, scale_modifier=1.0):
        """get_local_invisibility without its images -> (sum_invisibility, best_pose_c2w or None) (visibility.py)."""
        from . import visibility as VIS
        return VIS.local_invisibility_target(self.params, view_c2w, cluster_invisibility_threshold, scale_modifier)

    @torch.no_grad()
    def extract_mesh(self, voxel_size, trunc=None, bounds=None, frames="keyframes", min_weight=1.0, depth_max=float("inf")):
        """The map's surface as a `sensor.MeshScene` (volume.py; NEW, no reference counterpart): per keyframe one `render_rgbd` at its est_w2c
        -- the existing render path -- whose colour, depth and silhouette go into a `TsdfVolume` (`fuse_frames`: silhouette > the mapping
        sil_thres, depth / silhouette), then `TsdfVolume.extract_mesh(min_weight)`.  `trunc` defaults to 4 voxels; `bounds` ((x0, y0, z0),
        (x1, y1, z1)) to the box of the centres of the Gaussians with opacity >= 0.5 padded by trunc (one small copy to the host).  The mesh
        is in the mapper's world frame (frame 0's camera), the frame the judge's samples are given in.  `frames`: "keyframes" only."""
        from . import volume as VOL
        if frames != "keyframes":
            raise ValueError(f'frames must be "keyframes", got {frames!r}')
        if self.params is None or not self.keyframe_list:
            raise RuntimeError("extract_mesh needs a map with at least one keyframe")
        voxel_size = float(voxel_size)
        trunc = 4.0 * voxel_size if trunc is None else float(trunc)
        if bounds is None:
            means = self.params["means3D"].detach()
            keep = torch.sigmoid(self.params["logit_opacities"].detach().reshape(-1)) >= 0.5
            if not bool(keep.any()):
                raise RuntimeError("extract_mesh: no Gaussian with opacity >= 0.5 to take the bounds from")
            kept = means[keep]
            box = torch.stack([kept.min(0).values, kept.max(0).values]).double().cpu().numpy()
            lo, hi = box[0] - trunc, box[1] + trunc
        else:
            lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
        dims = tuple(max(1, int(np.ceil((hi[a] - lo[a]) / voxel_size))) for a in range(3))
        vol = VOL.TsdfVolume(lo, voxel_size, dims, trunc, device=self.device)
        sil_thres = float(self.cfg["mapping"]["sil_thres"])
        for first in range(0, len(self.keyframe_list), VOL.MAX_FRAMES):
            depths, colors, sils, poses = [], [], [], []
            for kf in self.keyframe_list[first:first + VOL.MAX_FRAMES]:
                im, depth, sil = self.render_rgbd(kf["est_w2c"])
                colors.append(im.reshape(3, self.H, self.W)); depths.append(depth.reshape(self.H, self.W)); sils.append(sil.reshape(self.H, self.W))
                poses.append(kf["est_w2c"].detach().cpu().numpy())
            VOL.fuse_frames(vol, depths, self._k_host, poses, colors, sils, sil_thres, depth_max)
        return vol.extract_mesh(min_weight)

    # -- no-grad consumers (reference: render_rgbd / get_*_invisibility, __init__.py:604-838) ----------------
    @torch.no_grad()
    def render_rgbd(self, w2c, scale_modifier=1.0, width=None, height=None, intrinsics=None):
        k = self._k_host if intrinsics is None else np.asarray(intrinsics)
        cfgv = dict(self.cfg["viz"], viz_w=width or self.W, viz_h=height or self.H)
        if self.cfg.get("fused_preprocess", False) and "rgb_colors" in self.params:
            # the map's PARAMETERS straight into the rasteriser (activations inside its per-Gaussian kernel, identity frame transform: the
            # view is the camera's): no activation launches, and none of the depth / silhouette "colours" every caller discards
            from . import rasterizer as R
            cam = setup_camera(cfgv["viz_w"], cfgv["viz_h"], k, w2c.cpu() if torch.is_tensor(w2c) else w2c, cfgv["viz_near"], cfgv["viz_far"],
                               scale_modifier=scale_modifier, device=self.device, bg=(1.0, 1.0, 1.0))
            p = self.params
            im, _radii, depth, opacity, _dsq = R.render_rgbd_raw(cam, p["means3D"].detach(), torch.empty(0, device=self.device), p["logit_opacities"].detach(),
                                                                 p["log_scales"].detach(), p["unnorm_rotations"].detach(), [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                                                                 colors_precomp=p["rgb_colors"].detach())
            return im, depth, opacity
        rv, dv = M.get_rendervars(self.params, w2c)
        im, depth, opacity, _ = M.render(w2c, k, rv, dv, cfgv, scale_modifier=scale_modifier, device=self.device,
                                         with_silhouette=False)
        return im, depth, opacity

    @torch.no_grad()
    def topdown_maps(self, world_center, world_shape, grid_shape, upper, lower, height=1000.0, scale_modifier=0.01):
        """The planner's free map and visible map (visualizer.py:923-965) of the current map in one fused raster pass: world_center = (x, z),
        world_shape = (metres along x, metres along z), grid_shape = (W, H) as `get_topdown_cam` takes them from `topdown_info`; the height
        band as the visualiser cuts it (upper = agent_head, lower = agent_foot - agent_foot_adjust).  -> topdown.TopdownMaps (device tensors)."""
        from . import topdown as TD
        cam = TD.topdown_camera(world_center, world_shape, grid_shape, height=height, scale_modifier=scale_modifier, device=self.device)
        return TD.topdown_maps(self.params, cam, upper, lower, scale_modifier=scale_modifier)

    @torch.no_grad()
    def roadmap(self, world_center, world_shape, grid_shape, upper, lower, agent_xz, agent_radius, node_spacing, node_y=0.0, height=1000.0,
                scale_modifier=0.01):
        """From the current map to the planner's candidate viewpoints without a map leaving the device (roadmap.py; a grid formulation of
        src/planner/planner.py:111-370, NOT its contour / scipy Voronoi / networkx chain): `topdown_maps(...)`, then `plan_roadmap` with the
        agent at the pixel that shows `agent_xz` = world (x, z), `agent_radius` and `node_spacing` in metres (converted with the finer of the
        two pixel scales; the spacing to a whole number of pixels, at least 1).  -> (Roadmap, positions float64 [K, 3] on the HOST: the
        nodes' world (x, node_y, z) -- what `global_invisibility_scores` takes; a second small copy, of the K pixel pairs)."""
        from . import roadmap as RM
        maps = self.topdown_maps(world_center, world_shape, grid_shape, upper, lower, height, scale_modifier)
        W, H = int(grid_shape[0]), int(grid_shape[1])
        px_per_m = max(W / float(world_shape[0]), H / float(world_shape[1]))
        r, c = (int(v) for v in np.rint(RM.world_to_pixel(agent_xz, world_center, world_shape, grid_shape, height)))
        if not (0 <= r < H and 0 <= c < W):
            raise ValueError(f"agent_xz {tuple(float(v) for v in agent_xz)} projects to pixel {(r, c)}, outside the {H} x {W} map")
        cell = min(RM.MAX_CELL, max(1, int(round(float(node_spacing) * px_per_m))))
        rm = RM.plan_roadmap(maps, (r, c), float(agent_radius) * px_per_m, cell)
        rm.world = dict(world_center=tuple(float(v) for v in world_center), world_shape=tuple(float(v) for v in world_shape), grid_shape=(W, H),
                        height=float(height))
        rm.px_per_m, rm.radius_px = px_per_m, float(agent_radius) * px_per_m
        xz = RM.pixel_to_world(rm.node_rc.cpu().numpy(), **rm.world)     # (K pixel pairs to the host: the scores take host positions)
        positions = np.stack([xz[:, 0], np.full(rm.K, float(node_y)), xz[:, 1]], 1)
        return rm, positions

    @torch.no_grad()
    def plan_step(self, view_c2w, world_center, world_shape, grid_shape, upper, lower, agent_radius, node_spacing, height=1000.0,
                  scale_modifier=0.01, max_clusters=256, policy=None):
        """One planning step: `roadmap(...)` with the agent at `view_c2w`'s position (nodes at its height), `global_invisibility_scores` of the
        nodes, and the node with the largest invisibility -- ties go to the smaller path length, then to the lower index (every node of a
        Roadmap is reachable: nodes are picked among the pixels its geodesic field reaches).  This greedy choice (policy=None, the default)
        is NOT the reference's stateful subregion policy.
        -> dict(roadmap, positions [K, 3], invisibility [K], volume [K], node, path_rc int32 [n, 2] (device), waypoints fp32 [n, 3] (device;
        world, agent to node, at the agent's height)); node = -1 and empty paths when there is no node.

        policy: a `policy.SubregionPolicy` makes the reference's hierarchical choice instead (planner_node.py:249-463; what of it is not
        restated -- the reweighting after exhaustion, escape plans, spline smoothing -- is listed in policy.py): roadmap -> `node_distances`
        -> `subregions` -> `nodes_in_horizon` -> `global_invisibility_scores` -> `node_scores` -> `policy.choose` -> `path_to` ->
        `shortcut_path`.  The agent's pixel is recorded as visited; `policy.arrive` / `policy.fail` are the caller's to call as the agent
        moves.  The way to a node is measured along the roadmap (`node_path_length` / 12 pixels).  The dict gains subregions (labels int32
        [K], host), scores (int32 [K], host), distances (D, device), shortcut_rc (int32 [m, 2], device: the agent's pixel, then the path
        from the farthest pixel a straight line reaches with 1.5 radii of clearance), safe (0-dim uint8, device), and waypoints follow
        shortcut_rc; path_rc stays the whole pixel path."""
        from . import roadmap as RM
        c2w = np.asarray(view_c2w.detach().cpu().numpy() if torch.is_tensor(view_c2w) else view_c2w, dtype=np.float64)
        agent_xz, node_y = (c2w[0, 3], c2w[2, 3]), float(c2w[1, 3])
        rm, positions = self.roadmap(world_center, world_shape, grid_shape, upper, lower, agent_xz, agent_radius, node_spacing, node_y, height,
                                     scale_modifier)
        out = dict(roadmap=rm, positions=positions, invisibility=np.zeros(0), volume=np.zeros(0), node=-1,
                   path_rc=torch.zeros(0, 2, dtype=torch.int32, device=self.device), waypoints=torch.zeros(0, 3, device=self.device))
        if rm.K == 0:
            return out
        if policy is not None:
            return self._plan_step_policy(out, policy, view_c2w, node_y, max_clusters)
        inv, vol = self.global_invisibility_scores(view_c2w, positions, max_clusters=max_clusters)
        length = rm.node_path_length().cpu().numpy()
        node = int(np.lexsort((np.arange(rm.K), length, -inv))[0])
        path = rm.path_to(node)
        xz = RM.pixel_to_world(path, **rm.world)
        out.update(invisibility=inv, volume=vol, node=node, path_rc=path,
                   waypoints=torch.stack([xz[:, 0], torch.full_like(xz[:, 0], node_y), xz[:, 1]], 1))
        return out

    def _plan_step_policy(self, out, policy, view_c2w, node_y, max_clusters):
        """plan_step's second half under a SubregionPolicy (the roadmap has nodes)"""
        from . import policy as PL
        from . import roadmap as RM
        rm, positions = out["roadmap"], out["positions"]
        out.update(PL.plan(rm, policy, lambda: self.global_invisibility_scores(view_c2w, positions, max_clusters=max_clusters), rm.px_per_m, rm.radius_px))
        if out["node"] >= 0:
            xz = RM.pixel_to_world(out["shortcut_rc"], **rm.world)
            out["waypoints"] = torch.stack([xz[:, 0], torch.full_like(xz[:, 0], node_y), xz[:, 1]], 1)
        return out

    @torch.no_grad()
    def invisibility(self, w2c, width=120, height=150, intrinsics=None):
        """1 - opacity, the quantity the planner scores view points with (__init__.py:739,795)."""
        _, _, opacity = self.render_rgbd(w2c, width=width, height=height, intrinsics=intrinsics)
        return 1.0 - opacity
