"""The planner's top-down maps -- free map and visible map -- from the map's parameters in one fused raster pass.

The reference's visualiser renders them every GUI tick (src/visualizer/visualizer.py:923-965) as two full raster passes through one camera
1000 m above the scene (`get_topdown_cam`, :1577-1601; `scale_modifier = 0.01`):

* free map    -- the Gaussians between the agent's head and foot (`__cut_gaussian_by_height`: clone, mask, compact five tensors), the raw
                 accumulated opacity, then `free = opacity <= 0.4`;
* visible map -- every Gaussian on a white background, to bytes, to grey (cv2.COLOR_RGB2GRAY), then `unseen = grey == 255`.

Both passes share camera, projection, tile rectangles and depth order, and a tile's in-band list is a subsequence of its full list.  Here one
per-Gaussian launch (activations inside, plus the height test), one binning / sort and one blend launch with two running states per pixel
produce all four results on the device (gs_preprocess_forward_topdown / gs_render_forward_topdown, include/gsplat_hip.h).  The only host
synchronisation is the one every render needs for its instance counters.  There is no CPU fallback and no backward.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import rasterizer as R
from .camera import setup_camera

#: `free = opacity <= 0.4` (visualizer.py:948), compared in fp32 inside the blend kernel
FREE_OPACITY_THRESHOLD = 0.4
#: bytes of the image state a tick needs: everything in front of the layout's final_T region
_TILE_RANGES_ONLY = operator.attrgetter("final_T")


class TopdownMaps(NamedTuple):
    free_opacity: torch.Tensor         # [H, W] float32: 1 - T over the in-band Gaussians
    free_map_binary: torch.Tensor      # [H, W] uint8:   free_opacity <= 0.4
    visible_rgb: torch.Tensor          # [H, W, 3] uint8: all Gaussians over the camera's background (white), (clamp(c, 0, 1) * 255) truncated
    visible_map_binary: torch.Tensor   # [H, W] uint8:   grey(visible_rgb) == 255


def rgb_to_grey_u8(rgb):
    """OpenCV's 8-bit COLOR_RGB2GRAY in its published fixed-point form, (4899 R + 9617 G + 1868 B + 8192) >> 14, on a uint8 [..., 3] numpy
    array or tensor -- what the blend kernel evaluates per pixel (host twin, for callers and tests)."""
    if torch.is_tensor(rgb):
        v = rgb.to(torch.int32)
        return ((4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14).to(torch.uint8)
    v = np.asarray(rgb).astype(np.int64)
    return ((4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14).astype(np.uint8)


def topdown_camera(world_center, world_shape, grid_shape, height=1000.0, scale_modifier=0.01, bg=(1.0, 1.0, 1.0), near=0.01, far=100, device=None):
    """The rasteriser settings of `get_topdown_cam` (visualizer.py:1577-1601): a camera `height` metres up the -y axis of the mapper's y-down
    world, looking along +y, above `world_center` = (x, z); field of view from the scene's extent `world_shape` = (width along x, height along
    z) in metres; `grid_shape` = (W, H) pixels; principal point at the integer image centre.  `bg` is the visible map's background (the
    reference: white; the free map's opacity does not depend on it)."""
    W, H = int(grid_shape[0]), int(grid_shape[1])
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float64)
    c2w[:3, 3] = [float(world_center[0]), -float(height), float(world_center[1])]
    fx, fy = W / (float(world_shape[0]) / height), H / (float(world_shape[1]) / height)      # fov2focal(2 atan(extent / 2 h), pixels)
    K = np.array([[fx, 0.0, W // 2], [0.0, fy, H // 2], [0.0, 0.0, 1.0]])
    return setup_camera(W, H, K, np.linalg.inv(c2w), near=near, far=far, scale_modifier=scale_modifier, bg=bg, device=device)


@torch.no_grad()
def topdown_maps(params, cam, upper, lower, scale_modifier=0.01):
    """params: the map's parameter dict (`means3D`, `rgb_colors`, `unnorm_rotations`, `logit_opacities`, `log_scales` [P, 3] or [P, 1]), read
    in place -- no clone, mask, compaction or activation pass; cam: `topdown_camera(...)` (any single-view settings work); the height band as
    the visualiser passes it to `__cut_gaussian_by_height`: upper = agent_head, lower = agent_foot - agent_foot_adjust -- a Gaussian is in
    band iff not (-y < upper or -y > lower), y its world-frame means3D[:, 1].  `scale_modifier` replaces the camera's (None: keep it).
    -> TopdownMaps of device tensors."""
    lib = _lib.get()
    means3D = params["means3D"].detach()
    device = means3D.device
    R._require_rocm(device)
    upper, lower = float(upper), float(lower)
    if upper != upper or lower != lower:
        raise ValueError("topdown_maps: the height band must not be NaN")
    if scale_modifier is not None and float(scale_modifier) != float(cam.scale_modifier):
        cam = cam._replace(scale_modifier=float(scale_modifier))
    _lib.poll_async_status()
    P = int(means3D.shape[0])
    means3D = R._f32(means3D, device)
    colors = R._f32(params["rgb_colors"].detach(), device)
    rots = R._f32(params["unnorm_rotations"].detach(), device)
    logit = R._f32(params["logit_opacities"].detach(), device)
    log_scales = R._f32(params["log_scales"].detach(), device)
    if colors.shape != (P, 3) or rots.shape != (P, 4) or logit.numel() != P or log_scales.dim() != 2 or log_scales.shape[0] != P or \
            log_scales.shape[1] not in (1, 3):
        raise ValueError("topdown_maps: means3D [P,3], rgb_colors [P,3], unnorm_rotations [P,4], logit_opacities [P,1], log_scales [P,1] or [P,3]")
    iso = 1 if log_scales.shape[1] == 1 else 0
    gcam, keep = R._camera(cam, device, 0)
    W, H = int(cam.image_width), int(cam.image_height)
    cap = R._capture_target()
    # (only the tile ranges of the image state are used -- its first region; a capture gets the whole layout so that it decodes as usual)
    fr = R._begin_frame(lib, device, P, W, H, image_bytes=None if cap is not None else _TILE_RANGES_ONLY)
    geom, image, radii, st = fr.geom, fr.image, fr.radii, fr.st
    _lib.check(lib.gs_preprocess_forward_topdown(C.byref(gcam), P, R._ptr(means3D), R._ptr(colors), R._ptr(logit), R._ptr(log_scales), R._ptr(rots),
                                                 iso, upper, lower, R._ptr(radii), R._ptr(geom), R._ptr(image), R._ptr(fr.d_num), R._ptr(fr.h_num), st))
    free_opacity = torch.empty(H, W, dtype=torch.float32, device=device)
    free_bin = torch.empty(H, W, dtype=torch.uint8, device=device)
    vis_rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
    vis_bin = torch.empty(H, W, dtype=torch.uint8, device=device)

    def launch(cap_d, cap_tile, binning_, plist_):
        _lib.check(lib.gs_render_forward_topdown(C.byref(gcam), P, cap_d, cap_tile, R._ptr(geom), R._ptr(binning_), R._ptr(plist_), R._ptr(image),
                                                 R._ptr(free_opacity), R._ptr(free_bin), R._ptr(vis_rgb), R._ptr(vis_bin), st))

    # the rasteriser's optimistic launch with a capacity stream of its own: the one host synchronisation of a tick is the wait for its two counters
    D, _max_tile, bl, binning, point_list = R._bin_and_render(lib, fr, ("topdown", P, W, H, device.index), P, W, H, launch, segmented_ok=True)
    if cap is not None:
        cap.update(geom=geom, image=image, binning=binning, point_list=point_list, gl=fr.gl, il=fr.il, bl=bl, D=D, P=P, W=W, H=H, radii=radii)
    return TopdownMaps(free_opacity, free_bin, vis_rgb, vis_bin)
