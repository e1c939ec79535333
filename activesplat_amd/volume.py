"""From the map to a mesh on the device: TSDF fusion of depth frames and surface extraction.

A NEW CAPABILITY with no reference counterpart: the SplaTAM family gets a mesh by fusing rendered depth into a TSDF with Open3D, offline;
Open3D is not a dependency here.  The arithmetic is this build's own (include/gsplat_hip.h states it: gs_tsdf_integrate, gs_tsdf_count,
gs_tsdf_emit) and is pinned to restatements kept with the tests (tests/volume_cases.py), not to the reference.

* `TsdfVolume`   -- tsdf / weight / colour on a regular grid, x fastest; `integrate` folds one frame or a batch of up to MAX_FRAMES frames in
                    with ONE sweep over the volume (the voxel state stays in registers across the frames of a batch; a batch gives the bits
                    of the same frames integrated one call at a time); `extract_mesh` runs marching tetrahedra on Kuhn's split of every cell
                    (count, scan, emit; one 8-byte copy of the two totals in between) -> a welded, watertight `sensor.MeshScene`;
* `fuse_frames`  -- the batched loop over any number of frames.

The depth frames may be rendered from the map (`SplatMapper.extract_mesh`) or come straight from the sensor.  The mesh goes to
`sensor.sample_surface` / `judge.mesh_distances` and `io.save_mesh_ply`.  No atomics anywhere: two runs give the same bytes.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import rasterizer as R
from .judge import _host_floats, _on

MAX_FRAMES = 16                       # frames per gs_tsdf_integrate call: the poses travel in the kernel arguments
MAX_SIZE = 16384                      # image sizes: 1 <= width, height <= 16384, as gs_depth_cloud


def _images(t, name, device, lead):
    """a contiguous fp32 [B, *lead-dims, H, W] tensor on `device` from one frame or a batch (None stays None) -> (tensor, was a single frame)"""
    if t is None:
        return None, False
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not _on(t, device):
        raise ValueError(f"{name} must be on {device}, got {t.device}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    single = t.dim() == 2 + lead
    if single:
        t = t[None]
    if t.dim() != 3 + lead or (lead and t.shape[1] != 3) or t.numel() == 0:
        shape = "[3, H, W] or [B, 3, H, W]" if lead else "[H, W] or [B, H, W]"
        raise ValueError(f"{name} must have shape {shape}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach(), single


class TsdfVolume:
    """A truncated signed distance volume on one device.  `origin` (3 HOST floats) is the corner of voxel (0, 0, 0); grid point (i, j, k) is the
    voxel centre origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_size.  `dims` = (nx, ny, nz), nx * ny * nz < 2^31.  `trunc`: the truncation
    distance in metres; `max_weight`: where a voxel's weight stops growing (>= 1).  Device tensors, x fastest:
      tsdf [nz, ny, nx] fp32, starts at 1;  weight [nz, ny, nx] fp32, starts at 0;  color [nz, ny, nx, 3] fp32, starts at 0."""

    def __init__(self, origin, voxel_size, dims, trunc, max_weight=64.0, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        R._require_rocm(self.device)
        self.origin = np.ascontiguousarray(_host_floats(origin, "origin", ((3,),)), dtype=np.float32)
        self.voxel_size, self.trunc, self.max_weight = float(voxel_size), float(trunc), float(max_weight)
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError(f"dims must be (nx, ny, nz) with every dimension >= 1 and nx * ny * nz < 2^31, got {dims}")
        if not (np.isfinite(self.origin).all() and 0.0 < self.voxel_size < math.inf and 0.0 < self.trunc < math.inf and 1.0 <= self.max_weight < math.inf):
            raise ValueError("origin must be finite, voxel_size and trunc positive and finite, max_weight at least 1 and finite")
        self.dims = dims
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=self.device)

    def _origin_ptr(self):
        return self.origin.ctypes.data_as(C.POINTER(C.c_float))

    @torch.no_grad()
    def integrate(self, depth, intrinsics, w2c, color=None, silhouette=None, sil_thres=0.99, depth_max=math.inf):
        """Fold one frame (`depth` [H, W], `w2c` 4x4 or 3x4) or a batch ([B, H, W], [B, 4, 4] or [B, 3, 4], B <= MAX_FRAMES) into the volume,
        in frame order, with one sweep over it.  depth, `color` ([3, H, W] or [B, 3, H, W], the rasteriser's planar layout, values as the
        volume should hold them) and `silhouette` ([H, W] or [B, H, W]) are contiguous fp32 device tensors; `intrinsics` (3x3, or fx, fy,
        cx, cy; pixel centres at integer coordinates, as `judge.depth_cloud`) and `w2c` (world-to-camera; camera x right, y down, z forward)
        are HOST values.  With `silhouette` a pixel counts only where silhouette > sil_thres and its depth is depth / silhouette (the
        rasteriser's depth image is not normalised).  Depths outside (0, depth_max] and NaNs are skipped.  The rule, step by step:
        include/gsplat_hip.h (gs_tsdf_integrate).  Without `color` the volume's colour is left as it is.  No host synchronisation."""
        d, single = _images(depth, "depth", self.device, 0)
        col, _ = _images(color, "color", self.device, 1)
        sil, _ = _images(silhouette, "silhouette", self.device, 0)
        B, H, W = (int(v) for v in d.shape)
        if B > MAX_FRAMES:
            raise ValueError(f"at most {MAX_FRAMES} frames per integrate call, got {B} (fuse_frames loops)")
        if not (1 <= W <= MAX_SIZE and 1 <= H <= MAX_SIZE):
            raise ValueError(f"image size {W} x {H} out of range (1 <= width, height <= {MAX_SIZE})")
        for t, name, shape in ((col, "color", (B, 3, H, W)), (sil, "silhouette", (B, H, W))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{name} must match depth: expected {list(shape)}, got {list(t.shape)}")
        k = _host_floats(intrinsics, "intrinsics", ((3, 3), (4,)))
        k4 = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]] if k.shape == (3, 3) else k, dtype=np.float32)
        m = _host_floats(w2c, "w2c", ((4, 4), (3, 4)) if single else ((B, 4, 4), (B, 3, 4)))
        m12 = np.ascontiguousarray(m.reshape((-1,) + m.shape[-2:])[:, :3].reshape(-1), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        nx, ny, nz = self.dims
        _lib.check(_lib.get().gs_tsdf_integrate(nx, ny, nz, self._origin_ptr(), self.voxel_size, self.trunc, self.max_weight, R._ptr(self.tsdf),
                                                R._ptr(self.weight), R._ptr(self.color), B, W, H, R._ptr(d), R._ptr(col), R._ptr(sil),
                                                k4.ctypes.data_as(fp), m12.ctypes.data_as(fp), float(sil_thres), float(depth_max),
                                                _lib.stream_ptr(self.device)))

    @torch.no_grad()
    def extract_arrays(self, min_weight=1.0):
        """The zero surface as arrays on the device -> (vertices fp32 [V, 3], triangles int32 [T, 3], colors fp32 [V, 3], interpolated from
        the volume's colour).  Marching tetrahedra on Kuhn's split of every cell whose eight corners have weight >= min_weight; vertices on
        edges, t = a / (a - b) from the end with the lower index, welded; the right-hand normal points from negative to positive tsdf, towards
        free space; vertices in (grid point, edge slot) order, triangles in (cell, tetrahedron, triangle) order, the same bytes every run.
        Triangles without area (a vertex at t == 0) are KEPT, so that the topology stays a manifold.  A volume with a dimension of 1 or
        without a valid cell gives empty arrays.  The rules: include/gsplat_hip.h (gs_tsdf_count, gs_tsdf_emit).  Count, scan, then ONE 8-byte
        copy of the two totals (which waits for the device), then emit."""
        lib, dev = _lib.get(), self.device
        nx, ny, nz = self.dims
        need = int(lib.gs_tsdf_extract_scratch_bytes(nx, ny, nz))
        if need == 0:
            raise ValueError(f"a volume of {nx} x {ny} x {nz} is too large to extract: 7 * nx * ny * nz must be below 2^31 (vertex indices are int32)")
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(lib.gs_tsdf_count(nx, ny, nz, R._ptr(self.tsdf), R._ptr(self.weight), float(min_weight), R._ptr(scratch), R._ptr(counts),
                                     _lib.stream_ptr(dev)))
        V, T = (int(v) for v in counts.tolist())                 # the one copy that waits for the device
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        colors = torch.empty(V, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
        if V or T:
            _lib.check(lib.gs_tsdf_emit(nx, ny, nz, self._origin_ptr(), self.voxel_size, R._ptr(self.tsdf), R._ptr(self.color), R._ptr(scratch), V, T,
                                        R._ptr(vertices) if V else None, R._ptr(colors) if V else None, R._ptr(triangles) if T else None,
                                        _lib.stream_ptr(dev)))
        return vertices, triangles, colors

    @torch.no_grad()
    def extract_mesh(self, min_weight=1.0):
        """`extract_arrays` as a `sensor.MeshScene` on the volume's device, in the volume's frame: vertex colours are the interpolated volume
        colours taken as values in [0, 1] and rounded half up to a grey level (clipped).  An empty volume gives a scene without triangles."""
        from .sensor import MeshScene
        vertices, triangles, colors = self.extract_arrays(min_weight)
        scene = object.__new__(MeshScene)                        # (the constructor would read the index range back: the kernels wrote it)
        scene.device = self.device
        scene.vertices, scene.triangles = vertices, triangles
        scene.vertex_colors = torch.floor(colors * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8)
        scene.capacities, scene.last_counts = {}, None
        scene._upload_textures(None, None, None)
        return scene


@torch.no_grad()
def fuse_frames(volume, depths, intrinsics, w2cs, colors=None, silhouettes=None, sil_thres=0.99, depth_max=math.inf):
    """Any number of frames into `volume`, MAX_FRAMES per sweep, in order: `depths` [N, H, W] (or a list of [H, W]), `w2cs` N HOST 4x4 or 3x4
    matrices, `colors` [N, 3, H, W] and `silhouettes` [N, H, W] (or lists) optional; the rest as `TsdfVolume.integrate`.  The result does
    not depend on how the frames fall into sweeps.  -> volume"""
    def stacked(x, lo, hi):
        if x is None:
            return None
        return x[lo:hi].contiguous() if torch.is_tensor(x) else torch.stack(list(x[lo:hi])).contiguous()
    n = len(depths)
    poses = np.stack([_host_floats(m, "w2cs", ((4, 4), (3, 4)))[:3] for m in w2cs]) if len(w2cs) else np.zeros((0, 3, 4))
    if len(poses) != n or any(x is not None and len(x) != n for x in (colors, silhouettes)):
        raise ValueError("depths, w2cs, colors and silhouettes must hold one entry per frame")
    for lo in range(0, n, MAX_FRAMES):
        hi = min(n, lo + MAX_FRAMES)
        volume.integrate(stacked(depths, lo, hi), intrinsics, poses[lo:hi], stacked(colors, lo, hi), stacked(silhouettes, lo, hi), sil_thres, depth_max)
    return volume
