"""Map-quality evaluation on the device: PSNR, depth error, SSIM, MS-SSIM per frame, and the trajectory error.

The reference measures its map in two places.  `report_progress` (src/mapper/splatam/utils/eval_helpers.py:153-264), called from inside the mapper
loop (src/mapper/splatam/__init__.py:483,499-505), reports PSNR, "Depth RMSE" and depth L1 of the current frame; `eval` (eval_helpers.py:409-625),
SplaTAM's end-of-run evaluation, re-renders every frame at its estimated pose, adds MS-SSIM, LPIPS and the trajectory error and writes psnr.txt,
rmse.txt, l1.txt, ssim.txt.  Both use two raster passes and a dozen small torch launches per frame, and `eval` moves both images to the host for
the 5-scale MS-SSIM.  Here a frame is ONE fused render plus ONE library call (gs_eval_frame: a handful of short launches, fixed-order fp64 sums,
include/gsplat_hip.h states every column's rule), and all rows are read back once:

* `frame_metrics`  -- the public primitive: one row of eight doubles for a rendered frame and its target;
* `MapEvaluator`   -- a device table of rows, `summary()` (the means the reference prints) and `write()` (its four text files);
* `evaluate_map`   -- the loop of `eval` over a sequence of frames, with the trajectory error;
* `align`, `evaluate_ate` -- Horn's closed form on the host in numpy fp64 (3 x n values: not device work).

Pinned to the imported reference (tests/golden/eval.npz): PSNR, depth RMSE / L1 in all three modes, calc_ssim, align / evaluate_ate.  NOT pinned:
MS-SSIM (the package the reference imports is not installed; the kernels follow its published definition) and `depth_rmse_l2` (this build's
quantity).  LPIPS is not provided (no AlexNet weights).

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import rasterizer as R
from .judge import _on

SIL_MASK, IMAGE_VALID_MASK, SSIM, MS_SSIM = 1, 2, 4, 8           # GS_EVAL_* of include/gsplat_hip.h
COLUMNS = ("psnr", "depth_rmse", "depth_l1", "ssim", "ms_ssim", "valid_pixels", "depth_rmse_l2", "reserved")
FILES = (("psnr.txt", 0), ("rmse.txt", 1), ("l1.txt", 2), ("ssim.txt", 4))        # eval_helpers.py:604-607 (ssim.txt holds the MS-SSIM)


def _image(t, name, channels, device=None, size=None):
    """a contiguous fp32 [channels, H, W] tensor ([H, W] also for one channel) on `device`, or an error that names the argument"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if device is not None and not _on(t, device):
        raise ValueError(f"{name} must be on {device}, got {t.device}")
    R._require_rocm(t.device)
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if channels == 1 and t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[0] != channels or t.numel() == 0 or (size is not None and tuple(t.shape[1:]) != size):
        want = f"[{channels}, {size[0]}, {size[1]}]" if size is not None else f"[{channels}, H, W]"
        raise ValueError(f"{name} must have shape {want}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach()


def _flags(sil_mask, image_valid_mask, ssim, ms_ssim):
    return (SIL_MASK if sil_mask else 0) | (IMAGE_VALID_MASK if image_valid_mask else 0) | (SSIM if ssim else 0) | (MS_SSIM if ms_ssim else 0)


def frame_layout(width, height, flags):
    """gs_eval_frame_layout -> _lib.GsEvalLayout (scratch bytes, level sizes, whether MS-SSIM is defined for the size)"""
    lay = _lib.GsEvalLayout()
    _lib.check(_lib.get().gs_eval_frame_layout(int(width), int(height), int(flags), C.byref(lay)))
    return lay


def _checked_frame(im, depth, silhouette, gt_im, gt_depth, flags, device=None, size=None):
    im = _image(im, "im", 3, device, size)
    size = tuple(im.shape[1:])
    depth = _image(depth, "depth", 1, im.device, size)
    silhouette = _image(silhouette, "silhouette", 1, im.device, size)
    gt_im = _image(gt_im, "gt_im", 3, im.device, size)
    gt_depth = _image(gt_depth, "gt_depth", 1, im.device, size)
    if flags & MS_SSIM and min(size) <= 160:
        raise ValueError(f"ms_ssim needs min(height, width) > 160 (five scales of an 11-tap valid window), got {size[0]} x {size[1]}")
    return im, depth, silhouette, gt_im, gt_depth


def _eval_frame(frame, sil_thres, flags, row, scratch):
    im, depth, silhouette, gt_im, gt_depth = frame
    H, W = int(im.shape[1]), int(im.shape[2])
    _lib.check(_lib.get().gs_eval_frame(W, H, R._ptr(im), R._ptr(depth), R._ptr(silhouette), R._ptr(gt_im), R._ptr(gt_depth), float(sil_thres),
                                        int(flags), R._ptr(row), R._ptr(scratch), _lib.stream_ptr(im.device)))


@torch.no_grad()
def frame_metrics(im, depth, silhouette, gt_im, gt_depth, sil_thres, sil_mask=False, image_valid_mask=True, ssim=True, ms_ssim=True):
    """One frame's row -> [8] float64 on the device (COLUMNS; include/gsplat_hip.h, gs_eval_frame, states each rule): `im` / `gt_im` [3, H, W],
    `depth` / `silhouette` / `gt_depth` [H, W] or [1, H, W], contiguous float32 device tensors.  sil_mask: differences only where silhouette >
    sil_thres (the reference's eval with mapping_iters == 0 and no new Gaussians; report_progress(tracking=True)); image_valid_mask: both images
    times gt_depth > 0 (eval does, report_progress does not).  Columns switched off are NaN; ms_ssim needs min(H, W) > 160.  No host
    synchronisation."""
    flags = _flags(sil_mask, image_valid_mask, ssim, ms_ssim)
    frame = _checked_frame(im, depth, silhouette, gt_im, gt_depth, flags)
    dev = frame[0].device
    lay = frame_layout(frame[0].shape[2], frame[0].shape[1], flags)
    row = torch.zeros(8, dtype=torch.float64, device=dev)
    scratch = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device=dev)
    _eval_frame(frame, sil_thres, flags, row, scratch)
    return row


class MapEvaluator:
    """A table of `capacity` rows on `device` for frames of one size.  `add_frame` writes the next row (one library call, no host wait); `rows()`
    reads the table once.  Adding past `capacity` raises."""

    def __init__(self, width, height, capacity, device=None):
        self.W, self.H, self.capacity = int(width), int(height), int(capacity)
        if self.W < 1 or self.H < 1:
            raise ValueError(f"width and height must be positive, got {width} x {height}")
        if self.capacity < 1:
            raise ValueError(f"capacity must be at least 1, got {capacity}")
        self.device = torch.device(device if device is not None else "cuda")
        R._require_rocm(self.device)
        _lib.get()
        self._rows = torch.zeros(self.capacity, 8, dtype=torch.float64, device=self.device)
        self._scratch = None
        self.frames = 0

    def reset(self):
        self._rows.zero_()
        self.frames = 0

    @torch.no_grad()
    def add_frame(self, im, depth, silhouette, gt_im, gt_depth, sil_thres, sil_mask=False, image_valid_mask=True, ssim=True, ms_ssim=True):
        """the arguments of `frame_metrics`; the row goes to the table"""
        if self.frames >= self.capacity:
            raise ValueError(f"the table is full: capacity {self.capacity} rows")
        flags = _flags(sil_mask, image_valid_mask, ssim, ms_ssim)
        frame = _checked_frame(im, depth, silhouette, gt_im, gt_depth, flags, self.device, (self.H, self.W))
        need = int(frame_layout(self.W, self.H, flags).total_bytes)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        _eval_frame(frame, sil_thres, flags, self._rows[self.frames], self._scratch)
        self.frames += 1

    def rows(self):
        """[frames, 8] float64 on the host (COLUMNS); ONE copy, which waits for the device"""
        return self._rows[:self.frames].cpu().numpy()

    def summary(self, rows=None):
        """the means the reference prints at the end of eval (eval_helpers.py:584-593) -> dict"""
        r = self.rows() if rows is None else rows
        mean = (lambda c: float(np.mean(r[:, c]))) if len(r) else (lambda c: float("nan"))
        return dict(frames=int(len(r)), avg_psnr=mean(0), avg_rmse=mean(1), avg_l1=mean(2), avg_ssim=mean(3), avg_ms_ssim=mean(4))

    def write(self, directory, rows=None):
        """psnr.txt, rmse.txt, l1.txt, ssim.txt as the reference's np.savetxt calls write them (eval_helpers.py:604-607; its ssim.txt holds the
        MS-SSIM, so does this one).  lpips.txt is not written: LPIPS is not provided."""
        r = self.rows() if rows is None else rows
        os.makedirs(directory, exist_ok=True)
        for name, col in FILES:
            np.savetxt(os.path.join(directory, name), r[:, col])


# ---- the trajectory error (eval_helpers.py:24-78): Horn's closed form on the host, numpy fp64 ----
def align(model, data):
    """Horn's closed-form alignment of two 3 x n trajectories -> (rot [3, 3], trans [3, 1], trans_error [n]): rot model + trans ~ data."""
    model, data = np.asarray(model, dtype=np.float64), np.asarray(data, dtype=np.float64)
    if model.ndim != 2 or model.shape[0] != 3 or model.shape != data.shape or model.shape[1] == 0:
        raise ValueError(f"model and data must both have shape [3, n], got {list(model.shape)} and {list(data.shape)}")
    mc, dc = model.mean(1, keepdims=True), data.mean(1, keepdims=True)
    Wm = (model - mc) @ (data - dc).T                              # the sum of the outer products
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1.0
    rot = U @ S @ Vh
    trans = dc - rot @ mc
    err = rot @ model + trans - data
    return rot, trans, np.sqrt(np.sum(err * err, 0))


def _w2c_host(m):
    return (m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m)).astype(np.float64)


def evaluate_ate(gt_w2c_list, est_w2c_list):
    """-> (mean translational error after alignment, its true RMSE).  The first value is what the reference returns and NAMES "ATE RMSE"
    (eval_helpers.py:61-78 takes the mean); the second is the root of the mean square."""
    if len(gt_w2c_list) != len(est_w2c_list) or len(gt_w2c_list) == 0:
        raise ValueError(f"gt_w2c_list and est_w2c_list must hold the same number (> 0) of poses, got {len(gt_w2c_list)} and {len(est_w2c_list)}")
    gt = np.stack([_w2c_host(m)[:3, 3] for m in gt_w2c_list]).T
    est = np.stack([_w2c_host(m)[:3, 3] for m in est_w2c_list]).T
    _, _, err = align(gt, est)
    return float(err.mean()), float(np.sqrt(np.mean(err * err)))


def _pose_column(params, idx):
    """the estimated w2c of frame idx on the host (eval_helpers.py:559-563)"""
    from . import mapping as M
    q = F.normalize(params["cam_unnorm_rots"][..., idx].detach().float().cpu())
    w2c = torch.eye(4)
    w2c[:3, :3] = M.build_rotation(q)
    w2c[:3, 3] = params["cam_trans"][..., idx].detach().float().cpu()
    return w2c


def selected_frames(num_frames, eval_every=1):
    """the frames eval looks at: time_idx == 0 or (time_idx + 1) % eval_every == 0 (eval_helpers.py:448)"""
    return [t for t in range(int(num_frames)) if t == 0 or (t + 1) % int(eval_every) == 0]


@torch.no_grad()
def render_frame(params, cam, time_idx, pose7=None):
    """ONE fused render of the map at pose column `time_idx` of the camera parameters -> (im [3, H, W], depth [1, H, W], silhouette [1, H, W]);
    the reference's two raster passes (colour; depth + silhouette) in one.  pose7: the column's (normalised quaternion, translation) when the
    caller still has it on the host; otherwise it is read from the parameters (one small copy, which waits for the device)."""
    dev = params["means3D"].device
    if pose7 is None:
        q = F.normalize(params["cam_unnorm_rots"][..., time_idx].detach().float().reshape(1, 4)).reshape(4).cpu()
        t = params["cam_trans"][..., time_idx].detach().float().reshape(3).cpu()
        pose7 = [float(v) for v in q.tolist()] + [float(v) for v in t.tolist()]
    im, _radii, depth, opacity, _dsq = R.render_rgbd_raw(cam, params["means3D"].detach(), torch.empty(0, device=dev), params["logit_opacities"].detach(),
                                                         params["log_scales"].detach(), params["unnorm_rotations"].detach(), pose7,
                                                         colors_precomp=params["rgb_colors"].detach())
    return im, depth, opacity


@torch.no_grad()
def evaluate_map(params, frames, intrinsics, first_frame_w2c, sil_thres, mapping_iters, add_new_gaussians, eval_every=1, ssim=True, ms_ssim=True):
    """The loop of the reference's `eval` (eval_helpers.py:409-625) over `frames` (dicts with `color` [3, H, W] in 0..1, `depth` [1, H, W] and,
    for the trajectory, `gt_w2c` 4 x 4 -- the input of SplatMapper.run): per evaluated frame ONE render at pose column time_idx and one
    gs_eval_frame into a device table; the silhouette mask is used iff mapping_iters == 0 and not add_new_gaussians, the images are always masked
    by the valid depth, as eval does.  Frames whose ground-truth pose holds NaN are left out of the trajectory (:555-566); without any `gt_w2c` the
    trajectory error is None.  -> dict(rows [n, 8] float64, frames (the evaluated indices), summary, ate (mean, the reference's figure),
    ate_rmse (the true RMSE), evaluator)."""
    from .camera import setup_camera
    frames = list(frames)
    if not frames:
        raise ValueError("frames must hold at least one frame")
    dev = params["means3D"].device
    H, W = int(frames[0]["color"].shape[1]), int(frames[0]["color"].shape[2])
    w2c0 = _w2c_host(first_frame_w2c)
    cam = setup_camera(W, H, np.asarray(_w2c_host(intrinsics))[:3, :3], w2c0, device=dev)
    picked = selected_frames(len(frames), eval_every)
    ev = MapEvaluator(W, H, len(picked), device=dev)
    sil_mask = int(mapping_iters) == 0 and not add_new_gaussians
    for t in picked:
        fr = frames[t]
        im, depth, sil = render_frame(params, cam, t)
        ev.add_frame(im.contiguous(), depth.contiguous(), sil.contiguous(), fr["color"].to(dev).float().contiguous(),
                     fr["depth"].to(dev).float().contiguous(), sil_thres, sil_mask=sil_mask, image_valid_mask=True, ssim=ssim, ms_ssim=ms_ssim)
    ate = ate_rmse = None
    if all("gt_w2c" in fr for fr in frames):
        gt_list, est_list = [_w2c_host(frames[0]["gt_w2c"])], [w2c0]
        for idx in range(1, len(frames)):
            g = _w2c_host(frames[idx]["gt_w2c"])
            if np.isnan(g).any():
                continue
            gt_list.append(g)
            est_list.append(_pose_column(params, idx))
        ate, ate_rmse = evaluate_ate(gt_list, est_list)
    rows = ev.rows()
    return dict(rows=rows, frames=picked, summary=ev.summary(rows), ate=ate, ate_rmse=ate_rmse, evaluator=ev)
