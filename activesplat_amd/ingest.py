"""Frame ingest on the device: the pre-processing of a sensor frame (src/mapper/splatam/__init__.py:341-376) as one upload and one kernel.

`frames.to_mapping_tensors` resizes on the host (a float64 numpy bilinear resize of the colour image, a nearest resize of the depth) and moves the
results with pageable copies, each of which ends in a stream synchronise: the host waits for everything the previous frame enqueued.  Here the raw
frame goes up once and `gs_frame_ingest` (include/gsplat_hip.h states both resize rules) writes the colour and depth tensors of one or two
resolutions in one launch:

* `ingest_frame`  -- the public primitive: device tensors in (uint8 [h,w,3], float32 [h,w]), a list of (color [3,H,W], depth [1,H,W]) out;
* `FrameIngest`   -- the upload: two slots of pinned host buffers (image, depth, pose floats) with device counterparts, filled alternately;
                     `put` copies into a slot with numpy, issues non-blocking copies on the current stream and calls `ingest_frame`.  The host
                     waits in one place only: before a slot is refilled, for the copies it issued two frames ago.

The values are, bit for bit, those `frames.to_mapping_tensors` gives on the same device: the grey levels come from `frames.resize_linear`'s own
arithmetic and their float values from a table built with the host path's operations (`level_table`).  A float image is not taken here: that case of
`to_mapping_tensors` stays a host path.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import rasterizer as R

MAX_SIZE = 16384                     # gs_frame_ingest: 1 <= width, height <= 16384 for the source and every output
POSE_FLOATS = 7 + 16                 # a slot's small buffer: quaternion (w,x,y,z), translation, and the frame's row-major 4x4 ground-truth w2c

_tables = {}


def level_table(device):
    """float32 [256] on `device`: the value of every grey level, computed as `frames.to_mapping_tensors` computes it (uint8 -> float, / 255, by
    torch on that device), once per device."""
    device = torch.device(device)
    key = (device.type, torch.cuda.current_device() if device.type == "cuda" and device.index is None else device.index)
    t = _tables.get(key)
    if t is None:
        t = _tables[key] = (torch.arange(256, dtype=torch.uint8, device=device).float() / 255).contiguous()
    return t


def _sizes(sizes):
    out = [(int(w), int(h)) for w, h in sizes]
    if len(out) not in (1, 2):
        raise ValueError(f"sizes must hold one or two (width, height) pairs, got {len(out)}")
    for w, h in out:
        if not (1 <= w <= MAX_SIZE and 1 <= h <= MAX_SIZE):
            raise ValueError(f"output size {w} x {h} out of range (1 <= width, height <= {MAX_SIZE})")
    return out


@torch.no_grad()
def ingest_frame(image_u8, depth, sizes):
    """image_u8 uint8 [h,w,3] and depth float32 [h,w], contiguous, on one ROCm device; sizes: one or two (width, height) pairs ->
    [(color [3,H,W] float32 in 0..1, depth [1,H,W] float32), ...], freshly allocated, from ONE launch on the current stream (bilinear colour
    rounded half up to a grey level, nearest depth with its bits copied: include/gsplat_hip.h, gs_frame_ingest).  No host synchronisation."""
    if not torch.is_tensor(image_u8) or not torch.is_tensor(depth):
        raise TypeError("ingest_frame takes torch tensors (FrameIngest.put uploads host arrays)")
    R._require_rocm(image_u8.device)
    if image_u8.dtype != torch.uint8:
        raise TypeError(f"image must be uint8, got {image_u8.dtype} (a float image takes frames.to_mapping_tensors, on the host)")
    if depth.dtype != torch.float32:
        raise TypeError(f"depth must be float32, got {depth.dtype}")
    if image_u8.dim() != 3 or image_u8.shape[2] != 3 or image_u8.numel() == 0:
        raise ValueError(f"image must have shape [h, w, 3], got {list(image_u8.shape)}")
    h, w = int(image_u8.shape[0]), int(image_u8.shape[1])
    if tuple(depth.shape) != (h, w):
        raise ValueError(f"depth must have shape [{h}, {w}], got {list(depth.shape)}")
    if depth.device != image_u8.device:
        raise ValueError(f"depth must be on {image_u8.device}, got {depth.device}")
    if not image_u8.is_contiguous() or not depth.is_contiguous():
        raise ValueError("image and depth must be contiguous")
    if w > MAX_SIZE or h > MAX_SIZE:
        raise ValueError(f"source size {w} x {h} out of range (1 <= width, height <= {MAX_SIZE})")
    sizes = _sizes(sizes)
    dev = image_u8.device
    outs = [(torch.empty(3, H, W, dtype=torch.float32, device=dev), torch.empty(1, H, W, dtype=torch.float32, device=dev)) for W, H in sizes]
    flat = (C.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])
    second = outs[1] if len(outs) == 2 else (None, None)
    _lib.check(_lib.get().gs_frame_ingest(w, h, R._ptr(image_u8), R._ptr(depth), R._ptr(level_table(dev)), len(sizes), flat,
                                          R._ptr(outs[0][0]), R._ptr(outs[0][1]), R._ptr(second[0]), R._ptr(second[1]), _lib.stream_ptr(dev)))
    return outs


class _Slot:
    def __init__(self, w, h, device):
        pin = device.type == "cuda"
        self.image = torch.empty(h, w, 3, dtype=torch.uint8, pin_memory=pin)
        self.depth = torch.empty(h, w, dtype=torch.float32, pin_memory=pin)
        self.pose = torch.zeros(POSE_FLOATS, dtype=torch.float32, pin_memory=pin)
        self.image_np, self.depth_np, self.pose_np = self.image.numpy(), self.depth.numpy(), self.pose.numpy()
        self.d_image = torch.empty(h, w, 3, dtype=torch.uint8, device=device)
        self.d_depth = torch.empty(h, w, dtype=torch.float32, device=device)
        self.d_pose = torch.zeros(POSE_FLOATS, dtype=torch.float32, device=device)
        self.event = torch.cuda.Event() if pin else None
        self.in_flight = False


class FrameIngest:
    """The upload of raw frames of one source size: `put` stages a frame in one of two slots (pinned host buffers on a GPU) and returns the
    frame's device tensors without waiting for the device.  All work goes to the stream that is current when `put` is called; use one stream.

    A slot's host buffers may be rewritten only when the copies issued from them have finished: an event is recorded behind a slot's copies
    and waited for before the slot is filled again, two frames later -- the only place the host may wait, and only if those copies are still
    in flight.  The slot's DEVICE staging buffers need no such care: the kernel that read them is ahead of the next copy on the stream.
    On the host-emulated test build ("cpu") nothing is pinned and there is no event; everything else is the same."""

    def __init__(self, src_width, src_height, sizes, device):
        self.device = torch.device(device)
        R._require_rocm(self.device)
        self.w, self.h = int(src_width), int(src_height)
        if not (1 <= self.w <= MAX_SIZE and 1 <= self.h <= MAX_SIZE):
            raise ValueError(f"source size {self.w} x {self.h} out of range (1 <= width, height <= {MAX_SIZE})")
        self.sizes = _sizes(sizes)
        self._slots = [_Slot(self.w, self.h, self.device) for _ in range(2)]
        self._next = 0
        level_table(self.device)

    def _on_device(self, t):
        return torch.is_tensor(t) and t.device.type == self.device.type and t.device.type != "cpu"

    @torch.no_grad()
    def put(self, image, depth, quat, position, gt_w2c=None):
        """image uint8 [h,w,3], depth [h,w] metres, quat (w,x,y,z), position (3), optionally the frame's 4x4 ground-truth w2c ->
        (outputs, quat_device [4], position_device [3], gt_w2c_device [4,4] or None), outputs = [(color [3,H,W], depth [1,H,W]), ...] in the order
        of `sizes`.  Host arrays are copied into the slot before `put` returns: the caller may overwrite them at once.  The outputs are fresh
        tensors; the pose tensors are views of the slot's device buffer and hold this frame's values until the slot is used again, two `put`s
        later (clone what must live longer).  Device tensors for image / depth are used as they are, without staging."""
        s = self._slots[self._next]
        self._next ^= 1
        if s.in_flight and s.event is not None:
            s.event.synchronize()            # the copies of two frames ago: normally long finished
        s.in_flight = False
        nb = s.event is not None
        if self._on_device(image):
            d_image = image
        else:
            a = image.numpy() if torch.is_tensor(image) else np.asarray(image)
            if a.dtype != np.uint8:
                raise TypeError(f"image must be uint8, got {a.dtype} (a float image takes frames.to_mapping_tensors, on the host)")
            if a.shape != (self.h, self.w, 3):
                raise ValueError(f"image must have shape [{self.h}, {self.w}, 3], got {list(a.shape)}")
            np.copyto(s.image_np, a)
            s.d_image.copy_(s.image, non_blocking=nb)
            d_image = s.d_image
        if self._on_device(depth):
            d_depth = depth
        else:
            a = depth.numpy() if torch.is_tensor(depth) else np.asarray(depth)
            if a.shape != (self.h, self.w):
                raise ValueError(f"depth must have shape [{self.h}, {self.w}], got {list(a.shape)}")
            np.copyto(s.depth_np, a, casting="same_kind")
            s.d_depth.copy_(s.depth, non_blocking=nb)
            d_depth = s.d_depth
        s.pose_np[0:4] = np.asarray(quat, dtype=np.float32).reshape(4)
        s.pose_np[4:7] = np.asarray(position, dtype=np.float32).reshape(3)
        if gt_w2c is not None:
            s.pose_np[7:23] = np.asarray(gt_w2c, dtype=np.float32).reshape(16)
        s.d_pose.copy_(s.pose, non_blocking=nb)
        if s.event is not None:
            s.event.record()
            s.in_flight = True
        outs = ingest_frame(d_image, d_depth, self.sizes)
        return outs, s.d_pose[0:4], s.d_pose[4:7], (s.d_pose[7:23].view(4, 4) if gt_w2c is not None else None)
