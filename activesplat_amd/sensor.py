"""Mesh RGB-D sensor on the device: the frame the reference takes from Habitat-sim (colour, planar depth, a pose; src/dataloader/dataloader.py:168-235),
produced from a vertex-coloured triangle mesh by ray casting on the compute path, and the mesh samples its judge needs
(scripts/judges/eval_actions.py:59-66).

Habitat-sim rasterises the scene mesh through OpenGL/EGL.  Here the same two images come from `gs_mesh_render` (include/gsplat_hip.h states the
rendering rule: fp32 edge functions evaluated with the lower vertex index first, two-sided, nearest hit, ties to the lower triangle index):

* `MeshScene`      -- the mesh on the device: vertices, triangles, vertex colours; uploaded and validated once;
* `render_mesh`    -- the public primitive: (colour uint8 [H,W,3], planar depth float32 [H,W], triangle id int32 [H,W]) at a world-to-camera pose;
* `MeshSensor`     -- fixed intrinsics and size; `.frame(X_WV)` takes the pose `SplatMapper.run_raw` takes and returns what `ingest.ingest_frame`
                      takes, so that `SplatMapper.run_sensor` goes sense -> ingest -> map without a pixel leaving the device;
* `sample_surface` -- area-weighted surface samples for `judge.CompletionJudge`.

Only the depth / colour sensor of the simulator is here: no textures (vertex colours, interpolated), no sensor noise, no far plane, no semantic
ids, no actions, physics or navmesh.  The rule is two-sided; whether Habitat's renderer culls back faces was not established (no Habitat here),
so a mesh seen from behind differs if it does.  Nothing was run against Habitat-sim.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import rasterizer as R
from .frames import OPENCV_TO_OPENGL
from .judge import _host_floats

MAX_SIZE = 16384                      # gs_mesh_render: 1 <= width, height <= 16384
MID_GREY = 128


def _as_tensor(a):
    if torch.is_tensor(a):
        return a.detach()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a)))


class MeshScene:
    """A triangle mesh on one device: `vertices` [V,3] floating point (world frame; kept as float32), `triangles` [T,3] of an integer type (kept
    as int32), `vertex_colors` [V,3] uint8 or None (mid-grey, 128).  Arrays or tensors; uploaded once, here.  Shapes, types and the index
    range 0 .. V-1 are checked at construction (the range check reads two integers back when the triangles are already on the device).
    `device`: where to keep it; default: the device of `vertices` if that is a tensor, the current ROCm device for an array.

    `capacities` remembers, per (width, height), how many tile-list entries the last `render_mesh` of this scene needed (see there)."""

    def __init__(self, vertices, triangles, vertex_colors=None, device=None):
        v, t = _as_tensor(vertices), _as_tensor(triangles)
        if device is None:
            device = v.device if torch.is_tensor(vertices) else torch.device("cuda")
        self.device = torch.device(device)
        R._require_rocm(self.device)
        if not v.dtype.is_floating_point:
            raise TypeError(f"vertices must be floating point, got {v.dtype}")
        if v.dim() != 2 or v.shape[1] != 3:
            raise ValueError(f"vertices must have shape [V, 3], got {list(v.shape)}")
        if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
            raise TypeError(f"triangles must be of an integer type, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"triangles must have shape [T, 3], got {list(t.shape)}")
        V, T = int(v.shape[0]), int(t.shape[0])
        if V >= 2 ** 31 or T >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 vertices and triangles")
        if T and (V == 0 or int(t.min()) < 0 or int(t.max()) >= V):
            raise ValueError(f"triangles index outside the vertices 0 .. {V - 1}")
        if vertex_colors is None:
            c = torch.full((V, 3), MID_GREY, dtype=torch.uint8, device=self.device)
        else:
            c = _as_tensor(vertex_colors)
            if c.dtype != torch.uint8:
                raise TypeError(f"vertex_colors must be uint8, got {c.dtype}")
            if tuple(c.shape) != (V, 3):
                raise ValueError(f"vertex_colors must have shape [{V}, 3], got {list(c.shape)}")
        self.vertices = v.to(device=self.device, dtype=torch.float32).contiguous()
        self.triangles = t.to(device=self.device, dtype=torch.int32).contiguous()
        self.vertex_colors = c.to(self.device).contiguous()
        self.capacities = {}
        self.last_counts = None           # (D, longest tile list) of the last render_mesh

    @property
    def num_vertices(self):
        return int(self.vertices.shape[0])

    @property
    def num_triangles(self):
        return int(self.triangles.shape[0])

    @torch.no_grad()
    def transformed(self, transform):
        """The same mesh in another frame: every vertex through the 4x4 (or 3x4) HOST matrix `transform`, computed in float64 on the device and
        rounded to float32 once; triangles and colours are shared, not copied.  With the world-to-camera matrix of frame 0 this puts the mesh,
        and `sample_surface` of it, into the frame `SplatMapper.judge` works in."""
        m = _host_floats(transform, "transform", ((4, 4), (3, 4)))
        rot = torch.from_numpy(np.ascontiguousarray(m[:3, :3])).to(self.device)
        off = torch.from_numpy(np.ascontiguousarray(m[:3, 3])).to(self.device)
        out = object.__new__(MeshScene)
        out.device = self.device
        out.vertices = (self.vertices.double() @ rot.T + off).float().contiguous()
        out.triangles, out.vertex_colors = self.triangles, self.vertex_colors
        out.capacities, out.last_counts = {}, None
        return out


def _pose(intrinsics, w2c):
    k = _host_floats(intrinsics, "intrinsics", ((3, 3), (4,)))
    k4 = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]] if k.shape == (3, 3) else k, dtype=np.float32)
    m = _host_floats(w2c, "w2c", ((4, 4), (3, 4)))
    return k4, np.ascontiguousarray(m[:3].reshape(12), dtype=np.float32)


@torch.no_grad()
def render_mesh(scene, intrinsics, w2c, width, height, near=0.01):
    """`scene` seen from the world-to-camera pose `w2c` (4x4 or 3x4; camera x right, y down, z forward: the inverse of the c2w
    `judge.depth_cloud` takes) through `intrinsics` (3x3, or fx, fy, cx, cy); both HOST values ->
      (color uint8 [height, width, 3], depth float32 [height, width], tri_id int32 [height, width])  on the scene's device:
    planar depth in metres (0 where no triangle is hit), the index of the triangle hit (-1), its interpolated vertex colour (0).  The rule is
    in include/gsplat_hip.h (gs_mesh_render); triangles nearer than `near` along z are not seen.

    The length D of the per-tile triangle lists depends on the mesh and the pose.  The call is made with the capacity remembered for this
    (scene, size) in `scene.capacities` (at first a guess from the triangle count) and the two counters it writes -- D and the longest list,
    8 bytes -- are copied to the host: THAT copy waits for the device, once per call.  If D exceeded the capacity the launch wrote no image;
    the call is repeated with room for D, and the capacity is remembered.  An image from a launch that ran out of room is never returned."""
    if not isinstance(scene, MeshScene):
        raise TypeError(f"scene must be a MeshScene, got {type(scene).__name__}")
    W, H = int(width), int(height)
    if not (1 <= W <= MAX_SIZE and 1 <= H <= MAX_SIZE):
        raise ValueError(f"image size {W} x {H} out of range (1 <= width, height <= {MAX_SIZE})")
    k4, m12 = _pose(intrinsics, w2c)
    fp = C.POINTER(C.c_float)
    lib, dev, T = _lib.get(), scene.device, scene.num_triangles
    capacity = int(scene.capacities.get((W, H), max(4096, 4 * T)))
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    tri_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    color = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)           # (read as unsigned)
    while True:
        layout = _lib.GsMeshLayout()
        _lib.check(lib.gs_mesh_render_layout(T, W, H, capacity, C.byref(layout)))
        scratch = torch.empty(int(layout.total_bytes), dtype=torch.uint8, device=dev)
        _lib.check(lib.gs_mesh_render(scene.num_vertices, R._ptr(scene.vertices) if T else None, T, R._ptr(scene.triangles) if T else None,
                                      R._ptr(scene.vertex_colors) if T else None, k4.ctypes.data_as(fp), m12.ctypes.data_as(fp), float(near), W, H,
                                      R._ptr(scratch), capacity, R._ptr(depth), R._ptr(tri_id), R._ptr(color), R._ptr(counts), _lib.stream_ptr(dev)))
        need, longest = (int(v) & 0xffffffff for v in counts.tolist())         # the one copy that waits for the device
        if need <= capacity:
            break
        if need == 0xffffffff:
            raise RuntimeError("render_mesh: the tile lists need 2^32 entries or more")
        capacity = min(0xfffffffe, need + need // 8)
    scene.capacities[(W, H)] = capacity
    scene.last_counts = (need, longest)
    return color, depth, tri_id


class MeshSensor:
    """The simulator's colour + depth sensor on `scene`, with fixed `intrinsics` (3x3, or fx, fy, cx, cy) and image size."""

    def __init__(self, scene, intrinsics, width, height, near=0.01):
        if not isinstance(scene, MeshScene):
            raise TypeError(f"scene must be a MeshScene, got {type(scene).__name__}")
        self.scene, self.width, self.height, self.near = scene, int(width), int(height), float(near)
        self.k4 = _pose(intrinsics, np.eye(4))[0]

    def w2c(self, X_WV):
        """The world-to-camera matrix `render_mesh` takes, from a sensor pose X_WV in the simulator's convention (camera x right, y UP, z
        BACKWARD -- what `SplatMapper.run_raw` takes): flip the camera's y and z, invert."""
        return OPENCV_TO_OPENGL @ np.linalg.inv(np.asarray(X_WV, dtype=np.float64))

    def frame(self, X_WV):
        """-> (image uint8 [height, width, 3], depth float32 [height, width]) on the device, at the sensor pose X_WV (4x4, HOST)."""
        color, depth, _ = render_mesh(self.scene, self.k4, self.w2c(X_WV), self.width, self.height, self.near)
        return color, depth


@torch.no_grad()
def sample_surface(scene, n, uniforms=None, generator=None, return_faces=False):
    """`n` points on the surface of `scene`, area-weighted -> float32 [n, 3] on the scene's device.  In torch, float64, rounded once at the end;
    no kernel of its own: it runs once per scene.  With u = `uniforms` [n, 3] in [0, 1) (drawn with `generator` when not given):
      face    searchsorted(cumsum(area), u0 * total area, right=True), clipped to T - 1
      point   (r1, r2) = (u1, u2), folded to (1 - r1, 1 - r2) when r1 + r2 > 1;  a + r1 (b - a) + r2 (c - a)
    Given `uniforms` the result is reproducible to the bit.  return_faces: -> (points, face int64 [n]).  This follows the published description of area-weighted triangle sampling (what
    trimesh.sample.sample_surface documents, which the reference's judge calls); trimesh is not installed and was NOT run against this."""
    if not isinstance(scene, MeshScene):
        raise TypeError(f"scene must be a MeshScene, got {type(scene).__name__}")
    n = int(n)
    if n < 0 or scene.num_triangles == 0:
        raise ValueError("sample_surface needs n >= 0 and a mesh with at least one triangle")
    dev = scene.device
    if uniforms is None:
        u = torch.rand(n, 3, dtype=torch.float64, generator=generator, device=generator.device if generator is not None else dev).to(dev)
    else:
        u = _as_tensor(uniforms).to(device=dev, dtype=torch.float64)
        if tuple(u.shape) != (n, 3):
            raise ValueError(f"uniforms must have shape [{n}, 3], got {list(u.shape)}")
    v = scene.vertices.double()
    tri = scene.triangles.long()
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    cum = torch.cumsum(area, 0)
    face = torch.searchsorted(cum, (u[:, 0] * cum[-1]).contiguous(), right=True).clamp(max=scene.num_triangles - 1)
    r1, r2 = u[:, 1], u[:, 2]
    fold = (r1 + r2) > 1.0
    r1, r2 = torch.where(fold, 1.0 - r1, r1), torch.where(fold, 1.0 - r2, r2)
    fa, fb, fc = a[face], b[face], c[face]
    points = (fa + r1[:, None] * (fb - fa) + r2[:, None] * (fc - fa)).float().contiguous()
    return (points, face) if return_faces else points
