"""Drop-in `GaussianRasterizationSettings` / `GaussianRasterizer` backed by the gfx950 HIP library.

Mirrors the Python API the reference imports from the (absent) `diff_gaussian_rasterization`
package -- imports at src/mapper/splatam/splatam.py:22-23, utils/recon_helpers.py:2,
utils/eval_helpers.py:18; settings construction utils/recon_helpers.py:14-27 and
splatam.py:416-429; calls splatam.py:208,212,338,430,431 with the keyword tensors of
utils/slam_helpers.py:131-138.  Contract:

    rasterizer = GaussianRasterizer(raster_settings=cam)            # cheap, constructed per call
    color, radii, depth, opacity = rasterizer(means3D=..., means2D=..., opacities=...,
                                              colors_precomp=... | shs=...,
                                              scales=..., rotations=... | cov3D_precomp=...)

`color` [3,H,W] is differentiable w.r.t. means3D, colors_precomp/shs, opacities, scales, rotations,
cov3D_precomp and the dummy `means2D` [P,3] (NDC-scaled screen-space gradient, read by the reference's
densifier at utils/slam_external.py:100-108).  `radii` [P] int32 (>0 <=> visible), `depth` [1,H,W]
(sum z*alpha*T) and `opacity` [1,H,W] (1 - T_final) are non-differentiable by default, which is all the reference
needs (they are only read under torch.no_grad(), splatam.py:414,430); GaussianRasterizer(raster_settings,
differentiable_outputs=("depth", "opacity")) opts in to their gradients.

All compute is in libgsplat_hip.so through the C ABI of include/gsplat_hip.h; there is no fallback.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import threading
from typing import NamedTuple

import torch
from torch import nn

from . import _lib


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


#: statistics of the most recent forward on this process (read by bench.py / tests).  Process-global and unsynchronised: with forwards
#: in flight on several threads it holds the numbers of whichever finished last -- informational, nothing in the product path reads it
last_stats = {"num_rendered": 0, "P": 0}
#: per (P, W, H, device): (pair capacity, tile-list capacity) guessed for the next frame's optimistic launch
_capacity = {}
#: set False to always size the binning workspace from the exact counts (one mid-pipeline host sync per forward)
optimistic = True

#: pinned host counter pairs (D, largest tile list), one per (thread, device, stream): the scan kernel stores straight into
#: them, so two forwards in flight -- another stream of a keyframe batch, the planner / visualiser thread of the reference's
#: threaded layout (SURVEY section 8b "Threading") -- must never share one
_tls = threading.local()
_capacity_lock = threading.Lock()


@contextlib.contextmanager
def capture():
    """`with capture() as state:` -- the state buffers of the forwards run inside the block by THIS thread (the last one wins) are put
    into `state` (geom / image / binning workspaces, point_list, their layouts, D, P, W, H; layouts in include/gsplat_hip.h) so that
    tests and bench.py can decode the integer artefacts.  render_views publishes its atlas the same way: P = the virtual row count, W = the
    atlas width, plus `radii` [P], `view_stride` and `rows_per_view`.  Nothing is retained outside a capture block: the reference's
    `debug=True` settings flag alone does not pin any buffer."""
    stack = getattr(_tls, "captures", None)
    if stack is None:
        stack = _tls.captures = []
    state = {}
    stack.append(state)
    try:
        yield state
    finally:
        stack.remove(state)


def _require_rocm(device):
    """The product path takes ROCm device tensors only (no CPU fallback)."""
    if device.type != "cuda":
        raise RuntimeError("activesplat_amd rasteriser needs ROCm device tensors (no CPU fallback)")


def _host_counters(device, stream_handle):
    pool = getattr(_tls, "pinned", None)
    if pool is None:
        pool = _tls.pinned = {}
    key = (device.index, stream_handle)
    buf = pool.get(key)
    if buf is None:
        if len(pool) >= 64:                              # short-lived streams: do not grow without bound
            pool.pop(next(iter(pool)))
        buf = pool[key] = torch.zeros(2, dtype=torch.int32).pin_memory()
    return buf


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t, device):
    if t is None:
        return None
    if t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _stream(device):
    return _lib.stream_ptr(device)


#: the two size-only layouts of a (P, W, H) frame: asked from the library once, not per frame
_layouts = {}


def _frame_layouts(lib, P, W, H):
    key = (P, W, H)
    hit = _layouts.get(key)
    if hit is None:
        gl = _lib.GsGeomLayout(); _lib.check(lib.gs_geom_layout(P, W, H, C.byref(gl)))
        il = _lib.GsImageLayout(); _lib.check(lib.gs_image_layout(W, H, C.byref(il)))
        if len(_layouts) >= 64:                          # P changes with every densify / growth step
            _layouts.pop(next(iter(_layouts)))
        hit = _layouts[key] = (gl, il, int(lib.gs_backward_scratch_bytes(P)))
    return hit


def _camera(rs: GaussianRasterizationSettings, device, sh_coeffs: int):
    keep = dict(bg=_f32(rs.bg, device).reshape(-1), view=_f32(rs.viewmatrix, device).reshape(-1),
                proj=_f32(rs.projmatrix, device).reshape(-1), campos=_f32(rs.campos, device).reshape(-1))
    if keep["view"].numel() != 16 or keep["proj"].numel() != 16 or keep["bg"].numel() != 3:
        raise Exception("GaussianRasterizationSettings: viewmatrix/projmatrix must hold 16 values, bg 3")
    cam = _lib.GsCamera(int(rs.image_width), int(rs.image_height), int(rs.sh_degree), int(sh_coeffs),
                        float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier), 0,
                        keep["bg"].data_ptr(), keep["view"].data_ptr(), keep["proj"].data_ptr(),
                        keep["campos"].data_ptr())
    return cam, keep


def _capture_target():
    """The dict the innermost capture() block of this thread publishes into, or None outside one."""
    caps = getattr(_tls, "captures", None)
    return caps[-1] if caps else None


#: what every frame launch starts from: the current stream (object -- None on the emulated build --, handle, c_void_p), the size-only
#: layouts, the fresh workspaces and the host counter pair
_Frame = collections.namedtuple("_Frame", "device cur st_handle st gl il scratch_bytes geom image radii d_num h_num")


def _begin_frame(lib, device, P, W, H, image_bytes=None):
    """image_bytes: None = the whole image layout, else a function of the layout -> bytes (topdown_maps uses its first region only)."""
    cur = torch.cuda.current_stream(device) if device.type == "cuda" else None     # ONE lookup per call (~6 us each)
    st_handle = int(cur.cuda_stream) if cur is not None else 0
    gl, il, scratch_bytes = _frame_layouts(lib, P, W, H)
    return _Frame(device, cur, st_handle, C.c_void_p(st_handle), gl, il, scratch_bytes,
                  torch.empty(gl.total_bytes, dtype=torch.uint8, device=device),
                  torch.empty(il.total_bytes if image_bytes is None else image_bytes(il), dtype=torch.uint8, device=device),
                  torch.empty(P, dtype=torch.int32, device=device), torch.empty(2, dtype=torch.int32, device=device),
                  _host_counters(device, st_handle) if cur is not None else torch.zeros(2, dtype=torch.int32))


def _capacity_guess(key):
    """(pair capacity, tile-list capacity) for the optimistic launch of `key`'s next frame; None: size it from the exact counts."""
    if key is None or not optimistic:
        return None
    with _capacity_lock:
        return _capacity.get(key)


def _capacity_update(key, D, max_tile):
    with _capacity_lock:
        old = _capacity.get(key, (0, 0))                    # monotone: views that alternate settle on the largest
        if len(_capacity) >= 64 and key not in _capacity:   # P changes with every densify / growth step: keep the table small
            _capacity.pop(next(iter(_capacity)))
        # (the tile-list bound only selects kernels and LDS variants: a tight margin keeps a 2 M-Gaussian frame -- lists of up to 4.8 k keys --
        # inside the one-workgroup bucket sort's 5632-key class; a list that outgrows it costs one exact re-launch)
        _capacity[key] = (max(old[0], int(D * 1.25) + 4096), max(old[1], max_tile + max_tile // 16 + 64))


def _record_launch(key, guess, hit, D, max_tile, P):
    """The bookkeeping of one finished frame launch.  key = None (render_views): an exact-size launch outside the capacity table -- no
    hit or miss is counted and nothing is stored (the atlas picks its segment count from the capacities)."""
    if key is not None:
        if hit:
            last_stats["optimistic_hits"] = last_stats.get("optimistic_hits", 0) + 1
        else:
            last_stats["optimistic_misses"] = last_stats.get("optimistic_misses", 0) + (1 if guess is not None else 0)
        _capacity_update(key, D, max_tile)
    last_stats["num_rendered"], last_stats["P"], last_stats["max_tile_instances"] = D, P, max_tile


def _render_at(lib, frame, W, H, launch, cap_d, cap_tile, bl=None):
    if bl is None:
        bl = _lib.GsBinLayout(); _lib.check(lib.gs_bin_layout(cap_d, cap_tile, W, H, C.byref(bl)))
    binning = torch.empty(bl.total_bytes, dtype=torch.uint8, device=frame.device)
    point_list = torch.empty(max(cap_d, 1), dtype=torch.int32, device=frame.device)
    launch(cap_d, cap_tile, binning, point_list)
    return bl, binning, point_list


def _bin_and_render(lib, frame, key, P, W, H, launch, segmented_ok=False):
    """Everything between "the per-Gaussian call is enqueued" and "the render that stands is known"; launch(cap_d, cap_tile, binning,
    point_list) issues the caller's one gs_render_forward* call.  -> (D, max_tile, bl, binning, point_list).

    Optimistic launch: the binning workspace is sized from the previous frame of this `key` (+25 %), the whole render is enqueued BEHIND
    the counting kernels, and only then does the host wait for the two counters -- the GPU keeps working through what used to be an idle
    gap (host wake-up + allocation + launch).  A frame whose true counts exceed the guess is re-launched with exact sizes (the render
    calls are capacity-safe and idempotent)."""
    cur, h_num = frame.cur, frame.h_num
    done = None
    guess = _capacity_guess(key)
    if guess is not None:
        if cur is not None:
            ev = torch.cuda.Event()
            ev.record(cur)
        bl_g = _lib.GsBinLayout(); _lib.check(lib.gs_bin_layout(guess[0], guess[1], W, H, C.byref(bl_g)))
        # Never optimistic where the capacities would CHOOSE the algorithm.  segmented_ok=False (the rasteriser): the segmented compositing of
        # few-tile images is switched on, and its segment count set, by the tile-list bound -- an inflated guess would make the image depend on
        # the call history; such frames take the exact launch, whose choice follows the true counts.  segmented_ok=True (topdown_maps): there
        # is no segmented top-down kernel, the streams kernel serves every tile count, so the bound decides nothing.
        if bl_g.path == 1 and (segmented_ok or bl_g.segments <= 1):
            done = _render_at(lib, frame, W, H, launch, guess[0], guess[1], bl_g)
        if cur is not None:
            ev.synchronize()                                # counters are on the host; the render is still in flight
    elif cur is not None:
        cur.synchronize()                                   # no guess (first frame of a stream, exact-size callers): D sizes the binning buffers
    D = int(h_num[0].item()) & 0xFFFFFFFF
    max_tile = int(h_num[1].item()) & 0xFFFFFFFF
    hit = done is not None and D <= guess[0] and max_tile <= guess[1]
    if not hit:
        done = _render_at(lib, frame, W, H, launch, D, max_tile)
    _record_launch(key, guess, hit, D, max_tile, P)
    return (D, max_tile) + done


class RawInputs(NamedTuple):
    """What the raw-parameter forward (render_rgbd_raw, render_rgbd_raw_direct) needs besides the tensors."""
    pose7: object                   # host (qw,qx,qy,qz,tx,ty,tz) of the frame's relative w2c; None with device_pose
    isotropic: bool                 # log_scales is [P,1]
    accumulate: bool = False        # the backward adds into the leaves' .grad
    visibility: object = None       # (max_2D_radius [P] float32, seen [P] bool), written by the forward kernel
    adam: object = None             # the optim.GaussianAdam whose step rides in the backward kernel
    gaussians_grad: bool = True     # False: the pose-only backward of tracking
    device_pose: object = None      # (cam_unnorm_rots [1,4,T], cam_trans [1,3,T], t): the kernels read column t in place


#: what the raw backward keeps of the forward's RawInputs: pose = (c_float * 7), None with a device pose; logit = the opacity parameters
_RawCtx = collections.namedtuple("_RawCtx", "pose iso accumulate logit")


#: the image outputs besides `color` that can carry a gradient, under their internal names; "silhouette" is render_rgbd's name for opacity
_OUTPUT_NAMES = {"depth": "depth", "opacity": "opacity", "silhouette": "opacity", "depth_sq": "depth_sq"}


def _output_request(differentiable_outputs, allowed, default, who):
    """The `differentiable_outputs` keyword -> None (the call's default: the very path and kernels of a call without the keyword) or a frozenset of
    internal names.  allowed: the names this entry point takes."""
    if isinstance(differentiable_outputs, str):
        differentiable_outputs = (differentiable_outputs,)
    names = tuple(differentiable_outputs)
    for n in names:
        if n not in allowed:
            raise ValueError(f"{who}: differentiable_outputs takes {sorted(allowed)}, not {n!r}")
    req = frozenset(_OUTPUT_NAMES[n] for n in names)
    return None if req == default else req


class _RasterizeGaussians(torch.autograd.Function):
    """fused=False: the reference contract (color differentiable; radii, depth, opacity not).
    fused=True : one pass also yields the reference's SECOND raster pass -- depth (differentiable), silhouette
                 (= opacity) and depth^2 -- see render_rgbd().
    outputs    : None, or the frozenset of {"depth", "opacity", "depth_sq"} that carry a gradient INSTEAD of that default
                 (differentiable_outputs= of the public calls); the others stay marked non-differentiable."""

    @staticmethod
    def forward(ctx, means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs, fused=False, raw=None,
                cam_rot=None, cam_trans=None, outputs=None):
        """raw = RawInputs: means3D / opacities / scales / rotations are the mapper's PARAMETERS (world-frame means, logit
        opacities, log scales, unnormalised quaternions); frame transform + activations run inside the per-Gaussian kernels (render_rgbd_raw).
        cam_rot [4] / cam_trans [3] (raw only): device tensors whose VALUES are pose7; the backward returns dL/d of them (gaussians_grad False:
        of them only -- the pose-only backward of tracking)."""
        lib = _lib.get()
        device = means3D.device
        leaves = (means3D, opacities, scales, rotations, colors_precomp)     # (raw + accumulate: the backward adds into these tensors' .grad)
        shs_in = shs
        _require_rocm(device)
        _lib.poll_async_status()                 # (a plain host load: did a chained backward of an earlier launch give up its wait?)
        P = int(means3D.shape[0])
        means3D = _f32(means3D, device)
        shs, colors_precomp = _f32(shs, device), _f32(colors_precomp, device)
        opacities, scales = _f32(opacities, device), _f32(scales, device)
        rotations, cov3D_precomp = _f32(rotations, device), _f32(cov3D_precomp, device)
        M = 0 if shs is None else int(shs.shape[1])
        cam, keep = _camera(rs, device, M)
        W, H = int(rs.image_width), int(rs.image_height)
        fr = _begin_frame(lib, device, P, W, H)
        st, geom, image, radii = fr.st, fr.geom, fr.image, fr.radii
        # camera-pose gradient (render_rgbd_raw(camera=...)): (pose_only, shape of cam_rot, shape of cam_trans)
        pose_req = None
        if raw is not None and cam_rot is not None and (cam_rot.requires_grad or cam_trans.requires_grad):
            pose_req = (not raw.gaussians_grad, cam_rot.shape, cam_trans.shape)
        ctx.pose_req = pose_req
        ctx.cam_inputs = cam_rot is not None         # the backward then owes autograd two more entries (None when the camera is frozen)
        ctx.outputs = outputs                        # (given: the call had all fourteen inputs, the backward owes one entry each)
        want_bwd = 1 if any(ctx.needs_input_grad[:8]) or pose_req is not None else 0
        pose = None
        ctx.devpose = raw.device_pose if raw is not None else None
        if raw is not None:
            iso = 1 if raw.isotropic else 0
            vis_max, vis_seen = raw.visibility if raw.visibility is not None else (None, None)
            tail = (_ptr(vis_max), _ptr(vis_seen), _ptr(radii), _ptr(geom), _ptr(image), _ptr(fr.d_num), _ptr(fr.h_num), want_bwd, st)
        if ctx.devpose is not None:
            # tracking (mapping.tracking_iteration): the pose is read by the kernels from cam_unnorm_rots[0, :, t] / cam_trans[0, :, t] in place
            rots_p, trans_p, t_idx = ctx.devpose
            _lib.check(lib.gs_preprocess_forward_raw_dev(C.byref(cam), P, _ptr(means3D), _ptr(shs), _ptr(colors_precomp), _ptr(opacities),
                                                         _ptr(scales), _ptr(rotations), _ptr(rots_p), _ptr(trans_p), int(rots_p.shape[-1]),
                                                         int(t_idx), iso, *tail))
        elif raw is not None:
            pose = (C.c_float * 7)(*[float(v) for v in raw.pose7])
            _lib.check(lib.gs_preprocess_forward_raw(C.byref(cam), P, _ptr(means3D), _ptr(shs), _ptr(colors_precomp), _ptr(opacities),
                                                     _ptr(scales), _ptr(rotations), pose, iso, *tail))
        else:
            _lib.check(lib.gs_preprocess_forward(C.byref(cam), P, _ptr(means3D), _ptr(shs), _ptr(colors_precomp),
                                                 _ptr(opacities), _ptr(scales), _ptr(rotations), _ptr(cov3D_precomp),
                                                 _ptr(radii), _ptr(geom), _ptr(image), _ptr(fr.d_num), _ptr(fr.h_num), want_bwd, st))
        color = torch.empty(3, H, W, dtype=torch.float32, device=device)
        depth = torch.empty(1, H, W, dtype=torch.float32, device=device)
        opacity = torch.empty(1, H, W, dtype=torch.float32, device=device)
        depth_sq = torch.empty(1, H, W, dtype=torch.float32, device=device) if fused else None
        # the backward's gradient records: allocated now (when a backward can follow) so that the blend kernel of this
        # forward zero-fills them as a side job instead of a fill launch in front of the backward
        scratch = None
        if want_bwd and P > 0:
            scratch = torch.empty(fr.scratch_bytes, dtype=torch.uint8, device=device)

        def launch(cap_d, cap_tile, binning_, plist_):
            _lib.check(lib.gs_render_forward(C.byref(cam), P, cap_d, cap_tile, _ptr(geom), _ptr(binning_), _ptr(plist_), _ptr(image),
                                             _ptr(color), _ptr(depth), _ptr(opacity), _ptr(depth_sq), _ptr(scratch), st))

        D, max_tile, bl, binning, point_list = _bin_and_render(lib, fr, (P, W, H, device.index), P, W, H, launch)
        ctx.rs, ctx.D, ctx.keep, ctx.fused, ctx.cam = rs, D, keep, fused, cam      # the backward reuses the camera block
        ctx.scratch, ctx.scratch_clean, ctx.sh_jac = scratch, scratch is not None, want_bwd
        ctx.has = (shs is not None, colors_precomp is not None, scales is not None, rotations is not None,
                   cov3D_precomp is not None)
        ctx.raw = None if raw is None else _RawCtx(pose, iso, bool(raw.accumulate), opacities)
        # in-kernel accumulation only into the very tensors the caller passed (a converted copy has no .grad to add to)
        adam = raw.adam if raw is not None else None
        same = raw is not None and (raw.accumulate or adam is not None) and all(a is b for a, b in zip(leaves, (means3D, opacities, scales, rotations, colors_precomp)))
        ctx.leaves = leaves if same else None
        ctx.adam = None
        if adam is not None:
            # the optimiser step inside the backward kernel: it updates the caller's parameter tensors in place
            if raw.accumulate:
                raise Exception("render_rgbd_raw: adam= and accumulate_grads= exclude each other")
            if pose_req is not None:
                raise Exception("render_rgbd_raw: adam= and a differentiable camera exclude each other (the library has no pose-gradient form of the "
                                "backward with the optimiser step)")
            if not same or (shs is not None and shs is not shs_in):
                raise Exception("render_rgbd_raw(adam=...): the parameters must be contiguous, 16-byte aligned fp32 tensors on the device (they are updated in place)")
            ctx.adam = (adam, leaves[:4] + (shs_in if shs_in is not None else leaves[4],))
        cap = _capture_target()
        if cap is not None:
            cap.update(geom=geom, image=image, binning=binning, point_list=point_list, gl=fr.gl, il=fr.il, bl=bl, D=D, P=P, W=W, H=H)
        e = torch.empty(0, device=device)
        ctx.save_for_backward(means3D, shs if shs is not None else e, colors_precomp if colors_precomp is not None else e,
                              scales if scales is not None else e, rotations if rotations is not None else e,
                              cov3D_precomp if cov3D_precomp is not None else e, radii, geom, point_list, image)
        ctx.set_materialize_grads(False)          # no zero-filled grad tensors for the non-differentiable outputs
        if outputs is not None:
            images = dict(depth=depth, opacity=opacity, depth_sq=depth_sq)
            ctx.mark_non_differentiable(radii, *[t for k, t in images.items() if t is not None and k not in outputs])
            return (color, radii, depth, opacity, depth_sq) if fused else (color, radii, depth, opacity)
        if fused:
            ctx.mark_non_differentiable(radii, opacity, depth_sq)
            return color, radii, depth, opacity, depth_sq
        ctx.mark_non_differentiable(radii, depth, opacity)
        return color, radii, depth, opacity

    @staticmethod
    def backward(ctx, grad_color, _gr=None, grad_depth=None, grad_opacity=None, grad_depth_sq=None):
        out = _RasterizeGaussians._backward(ctx, grad_color, grad_depth, grad_opacity, grad_depth_sq)
        if getattr(ctx, "cam_inputs", False) and len(out) == 11:
            out = out + (None, None)                     # camera tensors given but not differentiable (frozen pose)
        if getattr(ctx, "outputs", None) is not None:
            out = out + (None,) * (14 - len(out))
        return out

    @staticmethod
    def _backward(ctx, grad_color, grad_depth, grad_opacity=None, grad_depth_sq=None):
        lib = _lib.get()
        means3D, shs, colors, scales, rots, cov3Dp, radii, geom, point_list, image = ctx.saved_tensors
        has_sh, has_col, has_sc, has_rot, has_cov = ctx.has
        device = means3D.device
        P = int(means3D.shape[0])
        M = int(shs.shape[1]) if has_sh else 0
        cam = ctx.cam                                    # its device pointers are kept alive by ctx.keep
        if grad_color is None:
            grad_color = torch.zeros(3, int(ctx.rs.image_height), int(ctx.rs.image_width), device=device)
        grad_color = _f32(grad_color, device)
        outs = getattr(ctx, "outputs", None)
        depth_on = ctx.fused if outs is None else "depth" in outs
        grad_depth = _f32(grad_depth, device) if (depth_on and grad_depth is not None) else None
        # the opt-in image gradients (differentiable_outputs=): a backward that carries one goes through the *_grads entry points; every other
        # one -- a call with the keyword whose loss left those outputs alone included -- makes the same library call as before the keyword
        grad_opacity = _f32(grad_opacity, device) if (outs is not None and "opacity" in outs and grad_opacity is not None) else None
        grad_depth_sq = _f32(grad_depth_sq, device) if (outs is not None and "depth_sq" in outs and grad_depth_sq is not None) else None
        grads = None
        if grad_opacity is not None or grad_depth_sq is not None:
            grads = _lib.GsImageGrads(grad_color.data_ptr(), *[None if g is None else g.data_ptr() for g in (grad_depth, grad_opacity, grad_depth_sq)])
        scratch, clean = _take_scratch(ctx, lib, P, device)
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)  # noqa: E731  (kernel writes every row)
        pose_req = getattr(ctx, "pose_req", None)
        d_m2d = z(P, 3)
        if ctx.raw is not None:
            if ctx.adam == "stepped":
                # (retain_graph + a second backward through this render would apply the optimiser step twice, on already-stepped parameters)
                raise RuntimeError("render_rgbd_raw(adam=...): this render's backward has already applied its optimiser step; a second backward "
                                   "through the same graph is refused -- render again, or use accumulate_grads / a separate optimizer.step()")
            rc = ctx.raw
            # what every raw backward call starts with, has in its middle (after `accumulate` / before the parameter gradients) and ends on
            head = (C.byref(cam), P, ctx.D, _ptr(means3D), _ptr(shs if has_sh else None), _ptr(colors if has_col else None), _ptr(rc.logit),
                    _ptr(scales), _ptr(rots), rc.pose, rc.iso)
            mid = (_ptr(radii), _ptr(geom), _ptr(point_list), _ptr(image), _ptr(grad_color), _ptr(grad_depth), _ptr(d_m2d))
            if grads is not None:
                mid = mid[:4] + (C.byref(grads), mid[6])
            raw_backward = lib.gs_render_backward_raw if grads is None else lib.gs_render_backward_raw_grads
            pose_backward = lib.gs_render_backward_raw_pose if grads is None else lib.gs_render_backward_raw_pose_grads
            scr = (_ptr(scratch), 1 if clean else 0, int(ctx.sh_jac))
            if ctx.adam is not None:
                # single-keyframe step: Adam on the five per-Gaussian tensors rides in the per-Gaussian backward kernel (no gradient tensors)
                opt, tensors = ctx.adam
                desc = opt.backward_step_descriptors(tensors)                 # (validates, then advances the step counters ...; a refusal here
                ctx.adam = "stepped"                                          # leaves counters AND this graph as they were: the caller may retry)
                try:
                    _lib.check(lib.gs_render_backward_raw_adam(*head, *mid, *scr, desc, _stream(device)))
                except Exception:
                    opt.rollback_backward_step(tensors)                       # (... which a launch that did not happen must not keep)
                    ctx.adam = (opt, tensors)
                    raise
                # the parameters changed in place behind autograd's back: bump their version counters, so that any other graph that saved them
                # (a regulariser on the same parameters, a second keyframe rendered before this backward) fails loudly in ITS backward instead of
                # differentiating through stepped values -- and note that such a branch gets no rasteriser gradient from this render
                torch.autograd.graph.increment_version([t for t in tensors if t is not None])
                return None, d_m2d, None, None, None, None, None, None, None, None, None
            if pose_req is not None:
                d_pose = z(7)
                pscr = torch.empty(int(lib.gs_pose_grad_scratch_bytes(P)), dtype=torch.uint8, device=device)
                pose_tail = (d_pose[:4].view(pose_req[1]), d_pose[4:].view(pose_req[2]))
                if pose_req[0]:
                    # tracking: the pose gradient only -- no parameter gradient is formed (gs_render_backward_raw_pose, pose_only = 1)
                    _lib.check(pose_backward(*head, 0, *mid, None, None, None, None, None, None, *scr, 1, _ptr(d_pose), _ptr(pscr), _stream(device)))
                    return (None, d_m2d) + (None,) * 9 + pose_tail
        d_m3d, d_op = z(P, 3), z(P, 1)
        d_col = z(P, 3) if has_col else None
        d_shs = z(P, M, 3) if has_sh else None
        d_rot = z(P, 4) if has_rot else None
        if ctx.raw is not None:
            d_sc = z(P, 1 if rc.iso else 3)               # (gradients w.r.t. the parameters: log scales are [P,1] for an isotropic map)
            # accumulate: add into the leaves' .grad inside the kernel (what autograd would do with the results in separate passes);
            # leaves = (means3D, logit opacities, log scales, rotations, colours)
            leaves, acc, into = ctx.leaves, 0, None
            if leaves is not None:
                live = [x for x in leaves if x is not None]
                ok = all(x.is_leaf and x.requires_grad for x in live)
                have = [x.grad is not None and x.grad.is_contiguous() and x.grad.dtype == torch.float32 and x.grad.shape == x.shape for x in live]
                if ok and all(have):
                    acc, into = 1, [None if x is None else x.grad for x in leaves]
                elif ok and not any(x.grad is not None for x in live):
                    into = [None if x is None else torch.empty_like(x, memory_format=torch.contiguous_format) for x in leaves]
            if into is not None:
                d_m3d, d_op, d_sc, d_rot = into[0], into[1], into[2], into[3]
                if has_col:
                    d_col = into[4]
            args = (*head, acc, *mid, _ptr(d_m3d), _ptr(d_op), _ptr(d_col), _ptr(d_shs), _ptr(d_sc), _ptr(d_rot), *scr)
            tail = ()
            if pose_req is not None:
                # bundle adjustment: the same launch also reduces the camera-pose gradient (parameter gradients bit-identical to the plain call)
                _lib.check(pose_backward(*args, 0, _ptr(d_pose), _ptr(pscr), _stream(device)))
                tail = pose_tail
            else:
                _lib.check(raw_backward(*args, _stream(device)))
            if into is not None:
                if not acc:
                    for x, t in zip(leaves, into):
                        if x is not None:
                            x.grad = t
                return (None, d_m2d, d_shs, None, None, None, None, None, None, None, None) + tail
            return (d_m3d, d_m2d, d_shs, d_col, d_op, d_sc, d_rot, None, None, None, None) + tail
        d_sc = z(P, 3) if has_sc else None
        d_cov = z(P, 6) if has_cov else None
        image_grads = (_ptr(grad_color), _ptr(grad_depth)) if grads is None else (C.byref(grads),)
        _lib.check((lib.gs_render_backward if grads is None else lib.gs_render_backward_grads)(
            C.byref(cam), P, ctx.D, _ptr(means3D), _ptr(shs if has_sh else None), _ptr(colors if has_col else None),
            _ptr(scales if has_sc else None), _ptr(rots if has_rot else None), _ptr(cov3Dp if has_cov else None),
            _ptr(radii), _ptr(geom), _ptr(point_list), _ptr(image), *image_grads,
            _ptr(d_m2d), _ptr(d_m3d), _ptr(d_op), _ptr(d_col), _ptr(d_shs), _ptr(d_sc), _ptr(d_rot), _ptr(d_cov),
            _ptr(scratch), 1 if clean else 0, int(ctx.sh_jac), _stream(device)))
        return d_m3d, d_m2d, d_shs, d_col, d_op, d_sc, d_rot, d_cov, None, None, None


class _DirectCtx:
    """Stands in for an autograd context when a Function's forward / backward is called directly (render_rgbd_raw_direct, mapping.mapping_iteration)."""
    # one entry per input of _RasterizeGaussians.forward: the eight tensor inputs it asks about, then rs, fused, raw and the camera pair
    needs_input_grad = (True,) * 8 + (False,) * (_RasterizeGaussians.forward.__code__.co_argcount - 1 - 8)
    saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


def render_rgbd_raw_direct(rs, means3D, means2D, logit_opacities, log_scales, unnorm_rotations, raw, shs=None, colors_precomp=None):
    """render_rgbd_raw's forward without autograd (raw: RawInputs) -> (ctx for backward_direct / backward_pose_dev, (color, radii, depth,
    silhouette, depth_sq)); the caller has checked what render_rgbd_raw checks."""
    ctx = _DirectCtx()
    return ctx, _RasterizeGaussians.forward(ctx, means3D, means2D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, None, rs,
                                            True, raw)


def backward_direct(ctx, grad_color, grad_depth):
    """The backward of a render_rgbd_raw_direct forward -> the Function's gradient tuple ([1] is dL/dmeans2D)."""
    return _RasterizeGaussians._backward(ctx, grad_color, grad_depth)


def _take_scratch(ctx, lib, P, device):
    """-> (scratch, clean): the forward's zero-filled gradient records, or a dirty buffer of its own.  Released with this launch (64 B x P); a
    second backward through the same graph takes a fresh buffer plus a memset."""
    scratch, clean = ctx.scratch, ctx.scratch_clean
    if scratch is None:
        scratch, clean = torch.empty(int(lib.gs_backward_scratch_bytes(P)), dtype=torch.uint8, device=device), False
    ctx.scratch, ctx.scratch_clean = None, False
    return scratch, clean


def backward_pose_dev(ctx, grad_color, grad_depth, pose_scratch, d_pose=None):
    """The pose-only backward of a render whose forward read the pose from the device (RawInputs.device_pose, mapping.tracking_iteration):
    gs_render_backward_raw_pose_dev.  The per-workgroup pose rows go to pose_scratch (gs_pose_grad_scratch_bytes(P) bytes); d_pose [7] (optional)
    receives dL/d(qw,qx,qy,qz,tx,ty,tz) of the normalised column.  -> dL/dmeans2D [P,3]."""
    lib = _lib.get()
    means3D, shs, colors, scales, rots, _cov, radii, geom, point_list, image = ctx.saved_tensors
    has_sh, has_col = ctx.has[0], ctx.has[1]
    device = means3D.device
    P = int(means3D.shape[0])
    iso, logit = ctx.raw.iso, ctx.raw.logit
    rots_p, trans_p, t_idx = ctx.devpose
    scratch, clean = _take_scratch(ctx, lib, P, device)
    d_m2d = torch.empty(P, 3, dtype=torch.float32, device=device)
    _lib.check(lib.gs_render_backward_raw_pose_dev(
        C.byref(ctx.cam), P, ctx.D, _ptr(means3D), _ptr(shs if has_sh else None), _ptr(colors if has_col else None), _ptr(logit), _ptr(scales),
        _ptr(rots), _ptr(rots_p), _ptr(trans_p), int(rots_p.shape[-1]), int(t_idx), iso, _ptr(radii), _ptr(geom), _ptr(point_list), _ptr(image),
        _ptr(_f32(grad_color, device)), _ptr(None if grad_depth is None else _f32(grad_depth, device)), _ptr(d_m2d), _ptr(scratch),
        1 if clean else 0, int(ctx.sh_jac), _ptr(d_pose), _ptr(pose_scratch), _stream(device)))
    return d_m2d


#: the drop-in call goes through the C++ autograd front-end (csrc/torch_frontend.cpp: the same library calls in the same order as
#: _RasterizeGaussians above, without the interpreter in the way -- host time of a forward + backward ~240 -> ~90 us, which is what makes the reference's own
#: 256 x 256 frames GPU-bound).  False: the Python twin (A/B measurements, tests of the twin).  Inside a capture() block and on the
#: host-emulated test build the Python twin runs regardless.
use_frontend = True


#: the C++ front-end's encoding of an output request: -1 = the call's default, else a bit set
_OUTPUT_BITS = {"depth": 1, "opacity": 2, "depth_sq": 4}


def _frontend_apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs, fused, outputs=None):
    """The drop-in forward through the C++ front-end; None when this call is not one for it (then the Python twin takes it)."""
    if not use_frontend or _lib.emulated() or means3D.device.type != "cuda":
        return None
    cap = _capture_target()
    from . import _frontend
    _lib.get()                                          # (the HIP library itself missing: raises -- there is no CPU path)
    ext = _frontend.get_or_none()                       # (no g++ / torch headers on this box: ONE warning, then the Python twin -- the same library calls)
    if ext is None:
        return None
    device = means3D.device
    P, W, H = int(means3D.shape[0]), int(rs.image_width), int(rs.image_height)
    key = (P, W, H, device.index)
    guess = _capacity_guess(key)
    out, D, max_tile, hit, state, off = ext.rasterize(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs.bg,
                                                      rs.viewmatrix, rs.projmatrix, rs.campos, W, H, float(rs.tanfovx), float(rs.tanfovy),
                                                      float(rs.scale_modifier), int(rs.sh_degree), bool(fused), guess[0] if guess else 0,
                                                      guess[1] if guess else 0, cap is not None,
                                                      -1 if outputs is None else sum(_OUTPUT_BITS[k] for k in outputs))
    if cap is not None:
        # capture(): views of the one workspace (and of the exact re-render's buffers after a miss), under the names the Python twin publishes
        lib = _lib.get()
        gl, il, _ = _frame_layouts(lib, P, W, H)
        ws, binning, plist2 = state
        cap_d, cap_tile = (guess if hit else (D, max_tile))
        bl = _lib.GsBinLayout(); _lib.check(lib.gs_bin_layout(cap_d, cap_tile, W, H, C.byref(bl)))
        cap.update(geom=ws[off[0]:off[0] + off[1]], image=ws[off[2]:off[2] + off[3]], gl=gl, il=il, bl=bl, D=D, P=P, W=W, H=H, binning=binning,
                   point_list=ws[off[4]:off[4] + 4 * off[5]].view(torch.int32) if hit else plist2)
    _record_launch(key, guess, hit, D, max_tile, P)     # (the C++ front-end decides hits itself; the bookkeeping is the twin's)
    return tuple(out)


def rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                        raster_settings, differentiable_outputs=()):
    outputs = _output_request(differentiable_outputs, ("depth", "opacity"), frozenset(), "GaussianRasterizer") if differentiable_outputs else None
    out = _frontend_apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, raster_settings, False, outputs)
    if out is not None:
        return out
    if outputs is not None:
        return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, raster_settings,
                                         False, None, None, None, outputs)
    return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                     cov3D_precomp, raster_settings)


#: what render_rgbd / render_rgbd_raw take in differentiable_outputs, and their default
_FUSED_OUTPUTS = ("depth", "silhouette", "opacity", "depth_sq")
_FUSED_DEFAULT = frozenset(("depth",))


def render_rgbd(raster_settings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, differentiable_outputs=("depth",)):
    """Single-pass RGB + depth + silhouette render -- an ADDITIONAL entry point, the
    drop-in GaussianRasterizer is unchanged.

    The reference rasterises every training iteration twice on identical geometry: once for RGB and once with
    per-Gaussian "colours" [z_cam, 1, z_cam^2] (src/mapper/splatam/splatam.py:208,212 with
    utils/slam_helpers.py:196-249).  With the settings' viewmatrix equal to the w2c used for z_cam (true at every
    reference call site) those three channels are sum z*alpha*T, sum alpha*T and sum z^2*alpha*T of the SAME blend,
    so one pass returns
        color [3,H,W], radii [P], depth [1,H,W], silhouette [1,H,W], depth_sq [1,H,W]
    with `color` AND `depth` differentiable (the mapping loss back-propagates through both; silhouette and
    depth_sq are only used as masks / detached, splatam.py:213-231).  The depth gradient reaches means3D through
    the per-Gaussian view depth exactly as in the two-pass formulation.
    differentiable_outputs: which of "depth", "silhouette" and "depth_sq" carry a gradient (default: depth alone, as the reference's losses
    need).  With all three the pass is a complete differentiable replacement of the reference's second raster pass: a silhouette or
    free-space opacity loss, a depth-variance regulariser (depth_sq - depth^2).  The others stay marked non-differentiable.  A backward that
    carries dL/ddepth_sq walks images of few tiles with one walker per quadrant (the forward records no sum z^2 state for list segments)."""
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    outputs = _output_request(differentiable_outputs, _FUSED_OUTPUTS, _FUSED_DEFAULT, "render_rgbd")
    out = _frontend_apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, raster_settings, True, outputs)
    if out is not None:
        return out
    if outputs is not None:
        return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                         raster_settings, True, None, None, None, outputs)
    return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                     raster_settings, True)


def render_rgbd_raw(raster_settings, means3D, means2D, logit_opacities, log_scales, unnorm_rotations, pose7, shs=None, colors_precomp=None,
                    accumulate_grads=False, visibility=None, adam=None, camera=None, gaussians_grad=True, differentiable_outputs=("depth",)):
    """render_rgbd straight from the mapper's PARAMETERS: the frame transform + activations of transform_to_frame /
    transformed_params2rendervar (slam_helpers.py:252-304,124-139; `mapping.fused_rendervar` does them in two launches of their own) happen
    inside the per-Gaussian kernels of the rasteriser, forward and backward.  pose7 = host (qw,qx,qy,qz,tx,ty,tz) of the frame's relative
    w2c (camera quaternion normalised); log_scales [P,1] = isotropic map.  Colours given, or 16-coefficient SH rows.
    accumulate_grads (for `loss.backward()` over a batch of keyframes): the backward ADDS the gradients of means3D, logit_opacities,
    log_scales, unnorm_rotations and colors_precomp to those tensors' .grad inside its kernel and hands autograd nothing for them.
    visibility = (max_2D_radius [P] float32, seen [P] bool), both contiguous on the device: the mapper's statistics of this render
    (splatam.py:296-298: max_2D_radius = max(max_2D_radius, radius) in place, seen = radius > 0) written by the forward kernel itself.
    adam = the optim.GaussianAdam that owns the five tensors (single-keyframe steps -- the reference's loss.backward(); optimizer.step() on one
    frame, src/mapper/splatam/__init__.py:470-480): the backward kernel that forms a Gaussian's parameter gradients applies the Adam update
    to parameters and moments IN PLACE (gs_render_backward_raw_adam; same arithmetic as optimizer.step(), bit for bit) and writes no
    gradient tensors -- the five tensors keep .grad = None, a following optimizer.step() skips them; means2D.grad is delivered as usual.
    Not for gradient accumulation over several keyframes, and not on iterations whose densify / prune event replaces the tensors between
    backward and step (optim.densify_event).
    camera = (cam_rot [4], cam_trans [3]) device tensors (tracking / bundle adjustment, transform_to_frame(camera_grad=True)): the pose of the
    render -- cam_rot the NORMALISED camera quaternion (w,x,y,z), e.g. F.normalize(params['cam_unnorm_rots'][..., t]); torch differentiates that
    normalisation -- and autograd returns dL/dcam_rot, dL/dcam_trans from the same backward launch (gs_render_backward_raw_pose; a deterministic
    reduction, the parameter gradients bit-identical to the call without a camera).  dL/dcam_rot is the reference's: the rotation matrix
    is taken as build_rotation(cam_rot) (which renormalises) and the Gaussians' rotations as quat_mult(cam_rot, .), so the gradient is right
    for a unit-quaternion leaf passed as is as well as after F.normalize.  Camera tensors that do not require grad are a frozen pose (no pose
    reduction runs).  pose7 = None reads the values from the two tensors (one small device-to-host copy).  gaussians_grad=False (tracking): the pose gradient only -- the backward forms no parameter gradient and the
    Gaussian tensors (colours / SH rows included) receive none; means2D.grad and the visibility statistics are delivered as usual.  Not with adam=.
    differentiable_outputs: as for render_rgbd; works with accumulate_grads, camera= and gaussians_grad=False (the pose gradient rides on the same
    moments).  Not with adam=: the backward with the optimiser step inside has no form that takes dL/dsilhouette or dL/ddepth_sq."""
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    outputs = _output_request(differentiable_outputs, _FUSED_OUTPUTS, _FUSED_DEFAULT, "render_rgbd_raw")
    if adam is not None and outputs is not None and (outputs - _FUSED_DEFAULT):
        raise Exception("render_rgbd_raw: adam= takes differentiable_outputs=('depth',) only (the backward with the optimiser step inside "
                        "has no form for the silhouette / depth_sq gradients)")
    tail = () if outputs is None else (outputs,)
    if shs is not None and int(shs.shape[1]) != 16:
        raise Exception("render_rgbd_raw: SH rows of 16 coefficients only")
    iso = int(log_scales.shape[1]) == 1
    if visibility is not None:
        mx, seen = visibility
        P = int(means3D.shape[0])
        if not (mx.dtype == torch.float32 and mx.is_contiguous() and mx.numel() == P and seen.dtype == torch.bool and seen.is_contiguous()
                and seen.numel() == P and mx.device == means3D.device and seen.device == means3D.device):
            raise Exception("render_rgbd_raw: visibility = (float32 [P], bool [P]) contiguous tensors on the parameters' device")
    if camera is None:
        if not gaussians_grad:
            raise Exception("render_rgbd_raw: gaussians_grad=False is the pose-only backward: it needs camera=(cam_rot, cam_trans)")
        return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, None,
                                         raster_settings, True, RawInputs(pose7, iso, accumulate=accumulate_grads, visibility=visibility, adam=adam),
                                         *((None, None) + tail if tail else ()))
    cam_rot, cam_trans = camera
    if cam_rot.numel() != 4 or cam_trans.numel() != 3:
        raise Exception("render_rgbd_raw: camera = (cam_rot with 4 values, cam_trans with 3)")
    if adam is not None:
        raise Exception("render_rgbd_raw: adam= and a differentiable camera exclude each other (the library has no pose-gradient form of the "
                        "backward with the optimiser step)")
    if pose7 is None:
        pose7 = torch.cat([cam_rot.detach().reshape(4), cam_trans.detach().reshape(3)]).float().cpu().tolist()
    if not gaussians_grad:
        d = lambda t: None if t is None else t.detach()  # noqa: E731
        means3D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations = (d(means3D), d(shs), d(colors_precomp), d(logit_opacities),
                                                                                      d(log_scales), d(unnorm_rotations))
        accumulate_grads = False
    return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, logit_opacities, log_scales, unnorm_rotations, None,
                                     raster_settings, True, RawInputs(pose7, iso, accumulate=accumulate_grads, visibility=visibility, gaussians_grad=gaussians_grad),
                                     cam_rot, cam_trans, *tail)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings, differentiable_outputs=()):
        """differentiable_outputs: any of "depth", "opacity" -- those image outputs carry a gradient as well (an addition to the reference's
        contract, off by default: without it both stay marked non-differentiable)."""
        super().__init__()
        self.raster_settings = raster_settings
        _output_request(differentiable_outputs, ("depth", "opacity"), frozenset(), "GaussianRasterizer")      # (an unknown name fails here)
        self.differentiable_outputs = tuple(differentiable_outputs) if not isinstance(differentiable_outputs, str) else (differentiable_outputs,)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs,
                                   self.differentiable_outputs)


@torch.no_grad()
def render_views(settings_list, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                 return_atlas=False):
    """Forward-only render of V views of ONE set of Gaussians in a single pass (the planner's look-around panoramas,
    src/mapper/splatam/__init__.py:707-736, 765-778: three 120 x 150 views per node).  The views share size, fov, background,
    scale modifier and SH degree and differ in their view / projection matrices and camera centre.  The per-Gaussian stage runs
    once over V x P virtual Gaussians; binning, sorting and blending see ONE atlas image (GsCamera.num_views, gs_atlas_layout) --
    one set of launches and one host read of the counters instead of V.
    -> list of (color [3,H,W], radii [P] int32, depth [1,H,W], opacity [1,H,W]) per view (views of the atlas tensors; `radii` is the
       view's first P rows of the padded virtual layout -- each view owns ceil(P/256)*256 rows, the padding rows are never returned);
    return_atlas=True: (color [3,H,AW], depth [1,H,AW], opacity [1,H,AW], view_stride) -- view v is columns [v stride, v stride + W).
    Settings whose tensors live on the host (setup_camera(device="cpu")) cost ONE host-to-device copy for all views."""
    lib = _lib.get()
    V = len(settings_list)
    rs0 = settings_list[0]
    if V == 1:
        one = GaussianRasterizer(rs0)(means3D=means3D, means2D=None, opacities=opacities, shs=shs, colors_precomp=colors_precomp,
                                      scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
        return (one[0], one[2], one[3], int(rs0.image_width)) if return_atlas else [one]
    bg0 = [float(x) for x in rs0.bg.reshape(-1).tolist()]
    for rs in settings_list[1:]:
        if (rs.image_width, rs.image_height, rs.tanfovx, rs.tanfovy, rs.scale_modifier, rs.sh_degree) != \
                (rs0.image_width, rs0.image_height, rs0.tanfovx, rs0.tanfovy, rs0.scale_modifier, rs0.sh_degree) or \
                (rs.bg is not rs0.bg and [float(x) for x in rs.bg.reshape(-1).tolist()] != bg0):
            raise Exception("render_views: the views must share size, field of view, scale modifier, SH degree and background")
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    device = means3D.device
    _require_rocm(device)
    P, W, H = int(means3D.shape[0]), int(rs0.image_width), int(rs0.image_height)
    means3D, shs, colors_precomp = _f32(means3D, device), _f32(shs, device), _f32(colors_precomp, device)
    opacities, scales, rotations, cov3D_precomp = _f32(opacities, device), _f32(scales, device), _f32(rotations, device), _f32(cov3D_precomp, device)
    M = 0 if shs is None else int(shs.shape[1])
    if all(not rs.viewmatrix.is_cuda for rs in settings_list) and device.type == "cuda":
        host = torch.cat([torch.stack([rs.viewmatrix.reshape(16) for rs in settings_list]).reshape(-1),
                          torch.stack([rs.projmatrix.reshape(16) for rs in settings_list]).reshape(-1),
                          torch.stack([rs.campos.reshape(3) for rs in settings_list]).reshape(-1), rs0.bg.reshape(3).cpu()]).float()
        pack = host.to(device, non_blocking=True)
        keep = dict(pack=pack, view=pack[:16 * V], proj=pack[16 * V:32 * V], campos=pack[32 * V:35 * V], bg=pack[35 * V:35 * V + 3])
    else:
        keep = dict(bg=_f32(rs0.bg, device).reshape(-1),
                    view=torch.stack([_f32(rs.viewmatrix, device).reshape(16) for rs in settings_list]).contiguous(),
                    proj=torch.stack([_f32(rs.projmatrix, device).reshape(16) for rs in settings_list]).contiguous(),
                    campos=torch.stack([_f32(rs.campos, device).reshape(3) for rs in settings_list]).contiguous())
    cam = _lib.GsCamera(W, H, int(rs0.sh_degree), M, float(rs0.tanfovx), float(rs0.tanfovy), float(rs0.scale_modifier), V,
                        keep["bg"].data_ptr(), keep["view"].data_ptr(), keep["proj"].data_ptr(), keep["campos"].data_ptr())
    pv, aw, stride = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(lib.gs_atlas_layout(P, W, V, C.byref(pv), C.byref(aw), C.byref(stride)))
    Pv, AW, S = pv.value, aw.value, stride.value
    fr = _begin_frame(lib, device, max(Pv, 1), AW, H)
    geom, image, radii, st = fr.geom, fr.image, fr.radii, fr.st
    _lib.check(lib.gs_preprocess_forward(C.byref(cam), P, _ptr(means3D), _ptr(shs), _ptr(colors_precomp), _ptr(opacities), _ptr(scales),
                                         _ptr(rotations), _ptr(cov3D_precomp), _ptr(radii), _ptr(geom), _ptr(image), _ptr(fr.d_num), _ptr(fr.h_num), 0, st))
    color = torch.empty(3, H, AW, dtype=torch.float32, device=device)
    depth = torch.empty(1, H, AW, dtype=torch.float32, device=device)
    opacity = torch.empty(1, H, AW, dtype=torch.float32, device=device)

    def launch(cap_d, cap_tile, binning, plist):
        _lib.check(lib.gs_render_forward(C.byref(cam), P, cap_d, cap_tile, _ptr(geom), _ptr(binning), _ptr(plist), _ptr(image),
                                         _ptr(color), _ptr(depth), _ptr(opacity), None, None, st))

    # key = None: always at exact size and outside the capacity table (D and the longest tile list size the binning workspace)
    D, _, bl, binning, point_list = _bin_and_render(lib, fr, None, P, AW, H, launch)
    rows = Pv // V
    cap = _capture_target()
    if cap is not None:
        # the atlas as one frame of Pv virtual rows and AW columns (util.artefacts decodes it like any other), plus where a view sits in it:
        # view v owns rows [v rows, v rows + P) and columns [v stride, v stride + W)
        cap.update(geom=geom, image=image, binning=binning, point_list=point_list, gl=fr.gl, il=fr.il, bl=bl, D=D, P=max(Pv, 1), W=AW, H=H,
                   radii=radii, view_stride=S, rows_per_view=rows)
    if return_atlas:
        return color, depth, opacity, S
    return [(color[:, :, v * S:v * S + W], radii[v * rows:v * rows + P], depth[:, :, v * S:v * S + W], opacity[:, :, v * S:v * S + W])
            for v in range(V)]
