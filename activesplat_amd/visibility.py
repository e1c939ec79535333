"""The second half of the planner's visibility queries: clustering the look-around panoramas on the device, batched over Voronoi nodes.

The reference clusters the low-visibility pixels of every panorama with sklearn's DBSCAN on the host, inside the mapper class
(src/mapper/__init__.py:8-19 `get_convexhull_volume`: `1 - opacity > 0.8`, DBSCAN(eps=5, min_samples=25), once per Voronoi node --
src/visualizer/visualizer.py:991-995 loops `get_global_invisibility` over the nodes; src/mapper/__init__.py:92-117
`get_invisibility_clusters`: threshold 0.3, DBSCAN(eps=5, min_samples=10) on the 2 x downsampled panorama of the agent's own pose).
On a pixel grid DBSCAN is a disc-count stencil, a connected-component labelling of the core pixels and a border rule; `grid_dbscan` runs
them as HIP kernels (gs_grid_dbscan, include/gsplat_hip.h states the rule) and reproduces sklearn's labels exactly.

* `grid_dbscan`                 -- labels, cluster count, per-cluster {count, sum_row, sum_col, root, sum_value} and the image total;
* `look_around_nodes`           -- the panoramas of K nodes on the device: one activation, the 3 K views rendered up to 63 at a time;
* `global_invisibility_nodes`   -- per node what `get_convexhull_volume` holds after its DBSCAN line, ONE device-to-host copy for all nodes.  The
                                   dilate / findContours / ConvexHull loop behind it (OpenCV, scipy) stays with the caller;
* `cluster_hulls`               -- that loop on the device (gs_cluster_hulls): per cluster the dilated mask's outer border, its depths and the
                                   volume of their convex hull; per image the two sums `get_convexhull_volume` returns;
* `global_invisibility_scores`  -- the planner's whole global query: per node the two floats of `get_global_invisibility`, ONE small copy;
* `local_invisibility_target`   -- the whole of `get_local_invisibility` (src/mapper/splatam/__init__.py:762-837) without its images.
* `high_loss_grid`              -- the mask of `get_high_loss_samples` (src/mapper/splatam/__init__.py:212-215) and its cv2.resize to one pixel per
                                   degree (:218), one launch (gs_high_loss_grid; the header states the pixel rule and the integer resize rule);
* `high_loss_target`            -- the whole of `get_high_loss_samples` behind its render: that grid, `grid_dbscan`, ONE small device-to-host copy
                                   and `target_from_high_loss_clusters` (:219-250 from the cluster table) -> the pose turned to the largest cluster.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import lookaround as LA
from . import rasterizer as R
from .camera import setup_camera

#: most nodes one raster pass takes: gs_atlas_layout takes 64 views, a node has 3
MAX_NODES_PER_PASS = 21
#: nodes per raster pass by default.  A node's three views then sit in atlas slots 0-2, exactly where `look_around` renders them, and the
#: panoramas are bit-identical to per-node `look_around`.  In a later slot the view's pixel offset (128 per slot) is added to the projected
#: means in fp32 and rounded once (include/gsplat_hip.h, "THE SLOT RULE"); that rounding grows with the slot and is ALL that differs from a
#: single-view render.  Its smooth part stays inside the project's atlas bound scaled to 63 slots (opacity 1e-4 at slot 50); a few pixels per
#: pass flip a Gaussian's alpha >= 1/255 test and move by up to 1/255 (measured on the MI355X at 21 nodes per pass: opacity 3.9e-3, depth
#: 1.1e-2; profiles/visibility_clusters.txt), which is over that bound.  These pixels are predicted one by one by the slot-shifted fp64
#: reference of tests/atlas_cases.py (case `pano63`: all 63 slots, n_contrib equal at every pixel; profiles/README.md, "Atlas, view by view").
#: `nodes_per_pass=21` renders all 63 views in one pass for callers that accept a panorama that differs from per-node `look_around` there.
NODES_PER_PASS = 1
GLOBAL_THRESHOLD, GLOBAL_EPS, GLOBAL_MIN_SAMPLES = 0.8, 5, 25           # src/mapper/__init__.py:12, :18
GLOBAL_FOOTPRINT = (15, 15)                                             # src/mapper/__init__.py:38
GLOBAL_SKIP_DEPTH = 15.0                                                # :54
GLOBAL_VFOV_DEG = 150                                                   # :8 (the call site passes the intrinsics as `hfov`, which is unused: :64-65)
HULL_MAX_POINTS = 4096                                                  # contour points per cluster: the most gs_cluster_hulls takes (a 150 x 360 blob emits a few hundred)
HULL_OVERFLOW, HULL_NONFINITE, HULL_TRUNCATED, HULL_FACES = 1, 2, 4, 8  # status bits of gs_cluster_hulls
LOCAL_THRESHOLD, LOCAL_EPS, LOCAL_MIN_SAMPLES = 0.3, 5, 10              # src/mapper/__init__.py:93, :99
LOCAL_GATE = 100                                                        # src/mapper/splatam/__init__.py:809
LOCAL_SKIP_DEG = 15                                                     # :825
HIGH_LOSS_DEPTH_ERR, HIGH_LOSS_OPACITY = 0.3, 0.8                       # src/mapper/splatam/__init__.py:215
HIGH_LOSS_EPS, HIGH_LOSS_MIN_SAMPLES = 5, 10                            # :228
HIGH_LOSS_GATE = 20                                                     # :223
HIGH_LOSS_SKIP_DEG = 5                                                  # :248


class GridClusters(NamedTuple):
    labels: torch.Tensor        # [B, H, W] int32: -2 unmasked, -1 noise, else the cluster number (sklearn's)
    n_clusters: torch.Tensor    # [B] int32: the true count (may exceed max_clusters: the tables are then truncated, the labels are not)
    count: torch.Tensor         # [B, max_clusters] int32: pixels of the cluster, border pixels included
    sum_row: torch.Tensor       # [B, max_clusters] int32
    sum_col: torch.Tensor       # [B, max_clusters] int32
    root: torch.Tensor          # [B, max_clusters] int32: the cluster's smallest core pixel, row * W + col; -1 beyond n_clusters
    sum_value: torch.Tensor     # [B, max_clusters] float32: sum of the tested value (1 - v under complement) over the cluster
    total: torch.Tensor         # [B] float32: sum of the tested value over the whole image


@torch.no_grad()
def grid_dbscan(values, threshold, eps, min_samples, complement=False, max_clusters=256):
    """DBSCAN(eps, min_samples) on the pixels of `values` ([H, W] or [B, H, W] float32 device tensor; rows and images may be strided, the last
    dimension is dense) whose tested value -- v, or 1.0f - v with complement=True -- exceeds `threshold` in fp32.  -> GridClusters of device
    tensors (for an [H, W] input without the batch dimension).  No host synchronisation."""
    lib = _lib.get()
    if not torch.is_tensor(values) or values.dim() not in (2, 3):
        raise ValueError("grid_dbscan: values must be an [H, W] or [B, H, W] tensor")
    device = values.device
    R._require_rocm(device)
    single = values.dim() == 2
    v = values.detach()
    if single:
        v = v.unsqueeze(0)
    B, H, W = (int(s) for s in v.shape)
    if v.dtype != torch.float32:
        v = v.float()
    if min(B, H, W) > 0 and (v.stride(2) != 1 or v.stride(1) < W or v.stride(0) < 0 or v.data_ptr() % 4):
        v = v.contiguous()
    layout = _lib.GsDbscanLayout()
    _lib.check(lib.gs_grid_dbscan_layout(B, H, W, int(max_clusters), C.byref(layout)))
    M = int(max_clusters)
    ws = torch.empty(int(layout.total_bytes), dtype=torch.uint8, device=device)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=device)
    n_clusters = torch.empty(B, dtype=torch.int32, device=device)
    table = torch.empty(B, M, 4, dtype=torch.int32, device=device)
    sum_value = torch.empty(B, M, dtype=torch.float32, device=device)
    total = torch.empty(B, dtype=torch.float32, device=device)
    _lib.check(lib.gs_grid_dbscan(B, H, W, R._ptr(v), int(v.stride(1)), int(v.stride(0)), float(threshold), int(bool(complement)), int(eps),
                                  int(min_samples), M, R._ptr(ws), R._ptr(labels), R._ptr(n_clusters), R._ptr(table), R._ptr(sum_value),
                                  R._ptr(total), _lib.stream_ptr(device)))
    out = GridClusters(labels, n_clusters, table[..., 0], table[..., 1], table[..., 2], table[..., 3], sum_value, total)
    return GridClusters(*(t[0] for t in out)) if single else out


class NodePanoramas(NamedTuple):
    opacity: torch.Tensor       # [K, 150, 360] float32 (may be a strided view of the atlas gather)
    depth: torch.Tensor         # [K, 150, 360, 1] float32
    rgb: torch.Tensor           # [K, 150, 360, 3] uint8
    valid: tuple                # K bools: False for an all-zero position (opacity 1, depth 0, rgb 0 in that slot)

    def node(self, i):
        """node i's panorama as `look_around` returns it, or None for an all-zero position (the reference returns early)"""
        if not self.valid[i]:
            return None
        return {"opacity": self.opacity[i], "rgb": self.rgb[i], "depth": self.depth[i]}


def node_pose(view_c2w, position):
    """the camera of `get_global_invisibility` (src/mapper/splatam/__init__.py:701-704): x and z replaced, the camera height kept; None for the
    all-zero position"""
    position = np.asarray(position)
    assert position.shape == (3,), f"Position must be a numpy array with shape (3,), but got {position.shape}"
    if (position == np.zeros(3)).all():
        return None
    c2w = np.array(view_c2w, dtype=np.float64, copy=True)
    c2w[0, 3], c2w[2, 3] = position[0], position[2]
    return c2w


@torch.no_grad()
def look_around_nodes(params, view_c2w, positions, scale_modifier=1.0, nodes_per_pass=None):
    """The look-around panoramas of K nodes: `lookaround.look_around` at `node_pose(view_c2w, positions[k])` for every k, with ONE activation
    of the Gaussians for all nodes and one raster pass (rasterizer.render_views) per `nodes_per_pass` nodes (1..21; default NODES_PER_PASS,
    see there); nothing is copied to the host.  -> NodePanoramas, all on the device."""
    nodes_per_pass = NODES_PER_PASS if nodes_per_pass is None else int(nodes_per_pass)
    if not 1 <= nodes_per_pass <= MAX_NODES_PER_PASS:
        raise ValueError(f"look_around_nodes: nodes_per_pass must be 1..{MAX_NODES_PER_PASS} (an atlas holds 64 views)")
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    K = positions.shape[0]
    device = params["means3D"].device
    poses = [node_pose(view_c2w, p) for p in positions]
    valid = tuple(p is not None for p in poses)
    live = [k for k in range(K) if valid[k]]
    views = int(360 / LA.LOOK_HFOV_DEG)
    k3 = LA.look_around_k()
    parts = []
    if live:
        rv = LA._world_rendervar(params)
        rv.pop("means2D")
    for start in range(0, len(live), nodes_per_pass):
        chunk = live[start:start + nodes_per_pass]
        cams = [setup_camera(LA.LOOK_W, LA.LOOK_H, k3, np.linalg.inv(LA.rot_axis(poses[k], "y", np.deg2rad(LA.LOOK_HFOV_DEG * i))), LA.VIZ_NEAR,
                             LA.VIZ_FAR, scale_modifier=scale_modifier, device="cpu", bg=(1.0, 1.0, 1.0)) for k in chunk for i in range(views)]
        color, depth, opacity, stride = R.render_views(cams, return_atlas=True, **rv)
        n = len(chunk)
        cols = LA._panorama_columns(views * n, stride, device)           # [n * 360]: node j's panorama is columns [360 j, 360 (j + 1))
        op = opacity[0][:, cols].view(LA.LOOK_H, n, views * LA.LOOK_W).permute(1, 0, 2)
        dp = depth[0][:, cols].view(LA.LOOK_H, n, views * LA.LOOK_W).permute(1, 0, 2).unsqueeze(-1)
        im = (torch.clamp(color[:, :, cols], min=0, max=1.0) * 255).byte().view(3, LA.LOOK_H, n, views * LA.LOOK_W).permute(2, 1, 3, 0).contiguous()
        parts.append((op, dp, im))
    if len(parts) == 1 and len(live) == K:
        return NodePanoramas(parts[0][0], parts[0][1], parts[0][2], valid)
    PW = views * LA.LOOK_W
    opacity = torch.ones(K, LA.LOOK_H, PW, dtype=torch.float32, device=device)
    depth = torch.zeros(K, LA.LOOK_H, PW, 1, dtype=torch.float32, device=device)
    rgb = torch.zeros(K, LA.LOOK_H, PW, 3, dtype=torch.uint8, device=device)
    if live:
        index = torch.as_tensor(live, device=device)
        opacity[index] = torch.cat([p[0] for p in parts])
        depth[index] = torch.cat([p[1] for p in parts])
        rgb[index] = torch.cat([p[2] for p in parts])
    return NodePanoramas(opacity, depth, rgb, valid)


def _one_copy(tensors):
    """several device tensors -> their numpy arrays through ONE device-to-host copy"""
    flat = [t.contiguous().view(-1) for t in tensors]
    # (a one-element slice of a table counts as contiguous with its element stride still that of the table: restated with stride 1 for the byte view)
    flat = [(f.as_strided((f.numel(),), (1,)) if f.numel() == 1 else f).view(torch.uint8) for f in flat]
    host = torch.cat(flat).cpu().numpy()
    out, o = [], 0
    for t, f in zip(tensors, flat):
        n = f.numel()
        out.append(host[o:o + n].view(torch.empty(0, dtype=t.dtype).numpy().dtype).reshape(tuple(t.shape)))
        o += n
    return out


@torch.no_grad()
def global_invisibility_nodes(params, view_c2w, positions, scale_modifier=1.0, max_clusters=256, nodes_per_pass=None):
    """For every node of `positions` [K, 3], what `get_convexhull_volume` (src/mapper/__init__.py:8-19) holds after its DBSCAN line, for the
    panorama `get_global_invisibility` renders there: a list of K entries, None for an all-zero position, else a dict of numpy arrays
      depth [150, 360, 1], invisibility [150, 360] (= 1 - opacity, fp32), labels [150, 360] int32 (-2 where invisibility <= 0.8, -1 noise,
      else sklearn's cluster number), n_clusters, and per cluster (the first min(n_clusters, max_clusters)) count, sum_row, sum_col, root,
      sum_value; total = sum of the invisibility over the panorama.
    One activation, one raster pass per `nodes_per_pass` nodes (look_around_nodes), one clustering call and ONE device-to-host copy for all nodes."""
    pano = look_around_nodes(params, view_c2w, positions, scale_modifier, nodes_per_pass)
    K = len(pano.valid)
    if not any(pano.valid):
        return [None] * K
    g = grid_dbscan(pano.opacity, GLOBAL_THRESHOLD, GLOBAL_EPS, GLOBAL_MIN_SAMPLES, complement=True, max_clusters=max_clusters)
    depth, inv, labels, n, count, sr, sc, root, sv, total = _one_copy([pano.depth, 1.0 - pano.opacity, g.labels, g.n_clusters, g.count, g.sum_row,
                                                                        g.sum_col, g.root, g.sum_value, g.total])
    out = []
    for k in range(K):
        if not pano.valid[k]:
            out.append(None)
            continue
        m = min(int(n[k]), int(max_clusters))
        out.append(dict(depth=depth[k], invisibility=inv[k], labels=labels[k], n_clusters=int(n[k]), count=count[k, :m], sum_row=sr[k, :m],
                        sum_col=sc[k, :m], root=root[k, :m], sum_value=sv[k, :m], total=float(total[k])))
    return out


def ellipse_footprint(kh=15, kw=15):
    """OpenCV's getStructuringElement(MORPH_ELLIPSE, (kw, kh)) restated -> uint32 [kh], bit j of word i = cell (i, j): with r = kh // 2 and
    c = kw // 2, row i is the run of half-width round_half_even(c * sqrt((r * r - dy * dy) / (r * r))) around column c, dy = i - r (r = 0: the
    centre cell alone, as OpenCV computes it).  Not run against cv2 (include/gsplat_hip.h, gs_cluster_hulls)."""
    kh, kw = int(kh), int(kw)
    if not (1 <= kh <= 15 and 1 <= kw <= 15 and kh % 2 == 1 and kw % 2 == 1):
        raise ValueError("ellipse_footprint: kh and kw must be odd and in 1..15")
    r, c = kh // 2, kw // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    rows = np.zeros(kh, np.uint32)
    for i in range(kh):
        dy = i - r
        dx = int(round(c * np.sqrt((r * r - dy * dy) * inv_r2)))         # (Python's round: half to even, as cvRound)
        for j in range(max(c - dx, 0), min(c + dx + 1, kw)):
            rows[i] |= np.uint32(1 << j)
    return rows


class ClusterHulls(NamedTuple):
    volume: torch.Tensor            # [B, max_clusters] float64: the cluster's hull volume in the reference's units; 0 beyond n_clusters
    n_points: torch.Tensor          # [B, max_clusters] int32: emitted contour points (before the depth skips)
    sum_volume: torch.Tensor        # [B] float64: get_convexhull_volume's last_volume
    sum_invisibility: torch.Tensor  # [B] float64: its last_invisibility
    status: torch.Tensor            # [B] int32: HULL_* bits
    contour_xy: object              # [B, max_clusters, max_points, 2] int32 (x, y), zero behind a cluster's points; None unless asked for


@torch.no_grad()
def cluster_hulls(labels, depth, clusters, footprint=None, kw=None, skip_depth=GLOBAL_SKIP_DEPTH, x_scale=None, y_scale=None, max_points=HULL_MAX_POINTS,
                  contours=False):
    """The loop of `get_convexhull_volume` behind its DBSCAN line (src/mapper/__init__.py:29-90) for every cluster of every image, on the device
    (gs_cluster_hulls; include/gsplat_hip.h states the rule).  `labels` [B, H, W] (or [H, W]) and `clusters` are `grid_dbscan`'s result; `depth`
    is [B, H, W] or [B, H, W, 1] float32 on the same device (rows and images may be strided).  `footprint`: uint32 row bitmasks as
    `ellipse_footprint` returns them, `kw` columns wide (default: as wide as high; without a footprint the 15 x 15 ellipse); x_scale and
    y_scale default to the reference's deg2rad(360 / W) and deg2rad(150 / H).  `contours=True` also returns the contour points (for tests
    and debugging).  -> ClusterHulls of device tensors (without the batch dimension for [H, W] labels).  No host synchronisation."""
    lib = _lib.get()
    if not torch.is_tensor(labels) or labels.dim() not in (2, 3) or not torch.is_tensor(depth):
        raise ValueError("cluster_hulls: labels must be an [H, W] or [B, H, W] tensor and depth a tensor")
    device = labels.device
    R._require_rocm(device)
    single = labels.dim() == 2
    lab = labels.detach().unsqueeze(0) if single else labels.detach()
    B, H, W = (int(s) for s in lab.shape)
    d = depth.detach()
    if d.dim() == labels.dim() + 1 and d.shape[-1] == 1:
        d = d.squeeze(-1)
    if single and d.dim() == 2:
        d = d.unsqueeze(0)
    if tuple(d.shape) != (B, H, W) or d.device != device:
        raise ValueError(f"cluster_hulls: depth must be {B} x {H} x {W} (x 1) on the labels' device, got {tuple(depth.shape)}")
    if d.dtype != torch.float32:
        d = d.float()
    if min(B, H, W) > 0 and (d.stride(2) != 1 or d.stride(1) < W or d.stride(0) < 0 or d.data_ptr() % 4):
        d = d.contiguous()
    if lab.dtype != torch.int32 or not lab.is_contiguous():
        lab = lab.int().contiguous()
    n_clusters = clusters.n_clusters.reshape(-1).contiguous()
    sum_value = clusters.sum_value.reshape(B, -1).contiguous() if B > 0 else clusters.sum_value
    M = int(sum_value.shape[-1])
    if n_clusters.numel() != B or n_clusters.dtype != torch.int32 or sum_value.dtype != torch.float32:
        raise ValueError("cluster_hulls: clusters is not grid_dbscan's result for these labels")
    if footprint is None:
        footprint, kw = ellipse_footprint(*GLOBAL_FOOTPRINT), GLOBAL_FOOTPRINT[1]
    fp = np.ascontiguousarray(footprint, dtype=np.uint32).reshape(-1)
    kh = int(fp.shape[0])
    kw = kh if kw is None else int(kw)
    xs = np.deg2rad(360 / W) if x_scale is None else float(x_scale)
    ys = np.deg2rad(GLOBAL_VFOV_DEG / H) if y_scale is None else float(y_scale)
    P = int(max_points)
    layout = _lib.GsHullLayout()
    _lib.check(lib.gs_cluster_hulls_layout(B, H, W, M, P, C.byref(layout)))
    ws = torch.empty(int(layout.total_bytes), dtype=torch.uint8, device=device)
    volume = torch.empty(B, M, dtype=torch.float64, device=device)
    n_points = torch.empty(B, M, dtype=torch.int32, device=device)
    xy = torch.zeros(B, M, P, 2, dtype=torch.int32, device=device) if contours else None
    sum_volume = torch.empty(B, dtype=torch.float64, device=device)
    sum_invisibility = torch.empty(B, dtype=torch.float64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    _lib.check(lib.gs_cluster_hulls(B, H, W, R._ptr(lab), R._ptr(d), int(d.stride(1)), int(d.stride(0)), R._ptr(n_clusters), R._ptr(sum_value), M,
                                    fp.ctypes.data_as(C.POINTER(C.c_uint32)), kh, kw, float(skip_depth), xs, ys, P, R._ptr(ws), R._ptr(volume),
                                    R._ptr(n_points), R._ptr(xy) if contours else None, R._ptr(sum_volume), R._ptr(sum_invisibility), R._ptr(status),
                                    _lib.stream_ptr(device)))
    out = ClusterHulls(volume, n_points, sum_volume, sum_invisibility, status, xy)
    return ClusterHulls(*(t[0] if t is not None else None for t in out)) if single else out


@torch.no_grad()
def global_invisibility_scores(params, view_c2w, positions, scale_modifier=1.0, max_clusters=256, nodes_per_pass=None):
    """The planner's global query, finished on the device: for every node of `positions` [K, 3] the two floats `get_global_invisibility`
    (src/mapper/splatam/__init__.py:698-759) returns -- `get_convexhull_volume`'s (last_invisibility, last_volume) of the panorama rendered
    there -- as two float64 numpy arrays [K]; (0, 0) for an all-zero position, as the reference returns.  `look_around_nodes`, `grid_dbscan`,
    `cluster_hulls` and ONE device-to-host copy of [K] invisibility, [K] volume and [K] status.  Raises when a score would be silently
    truncated: a contour of more than HULL_MAX_POINTS points, more than `max_clusters` clusters in a panorama, or a hull that left its face
    bound (gs_cluster_hulls' status bits 0, 2, 3)."""
    pano = look_around_nodes(params, view_c2w, positions, scale_modifier, nodes_per_pass)
    K = len(pano.valid)
    if not any(pano.valid):
        return np.zeros(K), np.zeros(K)
    g = grid_dbscan(pano.opacity, GLOBAL_THRESHOLD, GLOBAL_EPS, GLOBAL_MIN_SAMPLES, complement=True, max_clusters=max_clusters)
    h = cluster_hulls(g.labels, pano.depth, g)
    inv, vol, status = _one_copy([h.sum_invisibility, h.sum_volume, h.status])
    valid = np.asarray(pano.valid)
    bad = valid & ((status & (HULL_OVERFLOW | HULL_TRUNCATED | HULL_FACES)) != 0)
    if bad.any():
        raise RuntimeError(f"global_invisibility_scores: nodes {np.nonzero(bad)[0].tolist()} have status {status[bad].tolist()} (1: a contour of more "
                           f"than {HULL_MAX_POINTS} points, 4: more than max_clusters={max_clusters} clusters, 8: hull face bound) -- the score would be truncated")
    return np.where(valid, inv, 0.0), np.where(valid, vol, 0.0)


def downsample2(image):
    """2 x area downsample of an [H, W] tensor with even H and W: ((a + b) + (c + d)) * 0.25f over each 2 x 2 block {a b; c d}, in fp32 and in
    that order (the reference: cv2.resize(..., INTER_AREA) at factor 0.5, src/mapper/splatam/__init__.py:810-813)."""
    a, b, c, d = image[0::2, 0::2], image[0::2, 1::2], image[1::2, 0::2], image[1::2, 1::2]
    return ((a + b) + (c + d)) * 0.25


def target_from_clusters(view_c2w, sum_invisibility, count, sum_row, sum_col, sum_value, cluster_invisibility_threshold):
    """src/mapper/splatam/__init__.py:809-830 on the host, from the cluster table of the downsampled panorama -> best_pose_c2w or None"""
    if not sum_invisibility > LOCAL_GATE:
        return None
    keep = [c for c in range(len(sum_value)) if sum_value[c] > cluster_invisibility_threshold]
    if not keep:
        return None
    best = keep[0]
    for c in keep[1:]:                                   # np.argmax: the first of equal maxima
        if sum_value[c] > sum_value[best]:
            best = c
    factor_width = factor_height = 0.5
    centre = (np.float64(sum_row[best]) / np.float64(count[best]), np.float64(sum_col[best]) / np.float64(count[best]))
    center_vec = np.array([centre[1] / factor_width - LA.LOOK_W / 2, centre[0] / factor_height - LA.LOOK_H / 2])
    horizontal_angle = np.deg2rad(center_vec[0])
    vertical_angle = np.deg2rad(center_vec[1])
    if np.abs(horizontal_angle) > np.deg2rad(LOCAL_SKIP_DEG) or np.abs(vertical_angle) > np.deg2rad(LOCAL_SKIP_DEG):
        return LA.rot_axis(LA.rot_axis(np.asarray(view_c2w, dtype=np.float64), "y", horizontal_angle), "x", vertical_angle)
    return None


@torch.no_grad()
def local_invisibility_target(params, view_c2w, cluster_invisibility_threshold=30, scale_modifier=1.0, max_clusters=256):
    """`get_local_invisibility` without its images -> (sum_invisibility, best_pose_c2w or None): the panorama at the agent's pose, sum(1 -
    opacity), and when that exceeds 100 the pose turned towards the centre of the downsampled panorama's most invisible cluster (clusters
    with sum > cluster_invisibility_threshold; the lowest cluster number wins a tie; None inside the 15-degree centre).  Everything up to
    the cluster table runs on the device whatever the sum; only the sum and the table are copied back, in one copy."""
    pano = LA.look_around(params, view_c2w, scale_modifier)
    inv = 1.0 - pano["opacity"]
    total = inv.sum().reshape(1)
    small = downsample2(inv)
    while True:
        g = grid_dbscan(small, LOCAL_THRESHOLD, LOCAL_EPS, LOCAL_MIN_SAMPLES, max_clusters=max_clusters)
        tot, n, count, sr, sc, sv = _one_copy([total, g.n_clusters.reshape(1), g.count, g.sum_row, g.sum_col, g.sum_value])
        if int(n[0]) <= max_clusters:
            break
        max_clusters = int(n[0])                         # (more clusters than rows in the table: once more with enough rows)
    m = int(n[0])
    return float(tot[0]), target_from_clusters(view_c2w, tot[0], count[:m], sr[:m], sc[:m], sv[:m], cluster_invisibility_threshold)


def _image(t, name):
    if not torch.is_tensor(t) or not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)):
        raise ValueError(f"high_loss_grid: {name} must be an [H, W] or [1, H, W] tensor")
    t = t.detach()
    t = t[0] if t.dim() == 3 else t
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


@torch.no_grad()
def high_loss_grid(render_depth, opacity, gt_depth, hfov=90, vfov=90):
    """The image half of `get_high_loss_samples` (src/mapper/splatam/__init__.py:212-218) in one launch: the mask `rendered depth > measured
    depth  and  |error| > 0.3 m (measured pixels only)  and  opacity > 0.8` and its cv2.resize(INTER_LINEAR) to hfov x vfov pixels in exact
    integers (gs_high_loss_grid, include/gsplat_hip.h states both rules).  The three images are [H, W] or [1, H, W] device tensors (strided ones
    are made contiguous).  -> (mask_full bool [H, W], grid float32 [vfov, hfov] of 0.0 / 1.0), on the device.  No host synchronisation."""
    lib = _lib.get()
    d, o, g = _image(render_depth, "render_depth"), _image(opacity, "opacity"), _image(gt_depth, "gt_depth")
    device = d.device
    R._require_rocm(device)
    if o.device != device or g.device != device or o.shape != d.shape or g.shape != d.shape:
        raise ValueError("high_loss_grid: render_depth, opacity and gt_depth must have one shape and one device")
    H, W = (int(n) for n in d.shape)
    gw, gh = int(hfov), int(vfov)
    mask = torch.empty(max(H, 0), max(W, 0), dtype=torch.uint8, device=device)
    grid = torch.empty(max(gh, 0), max(gw, 0), dtype=torch.float32, device=device)
    _lib.check(lib.gs_high_loss_grid(W, H, R._ptr(d), R._ptr(o), R._ptr(g), HIGH_LOSS_DEPTH_ERR, HIGH_LOSS_OPACITY, gw, gh, R._ptr(mask), R._ptr(grid),
                                     _lib.stream_ptr(device)))
    return mask.view(torch.bool), grid


def target_from_high_loss_clusters(view_c2w, total, count, sum_row, sum_col, cluster_invisibility_threshold, hfov=90, vfov=90):
    """src/mapper/splatam/__init__.py:219-250 on the host, from the cluster table of the grid -> high_loss_samples_pose_c2w or None.  `total` is
    the number of ones in the grid (np.sum of the resized mask: the "no points" return and the > 20 gate); a cluster's `invisibility_sum` is
    the sum of a 0 / 1 mask over its pixels, its count."""
    if not total > HIGH_LOSS_GATE:
        return None
    keep = [c for c in range(len(count)) if count[c] > cluster_invisibility_threshold]
    if not keep:
        return None
    best = keep[0]
    for c in keep[1:]:                                   # np.argmax: the first of equal maxima
        if count[c] > count[best]:
            best = c
    centre = (np.float64(sum_row[best]) / np.float64(count[best]), np.float64(sum_col[best]) / np.float64(count[best]))
    center_vec = np.array([centre[1] / hfov * hfov - hfov / 2, centre[0] / vfov * vfov - vfov / 2])
    horizontal_angle = np.deg2rad(center_vec[0])
    vertical_angle = np.deg2rad(center_vec[1])
    if np.abs(horizontal_angle) > np.deg2rad(HIGH_LOSS_SKIP_DEG) or np.abs(vertical_angle) > np.deg2rad(HIGH_LOSS_SKIP_DEG):
        return LA.rot_axis(LA.rot_axis(np.asarray(view_c2w, dtype=np.float64), "y", horizontal_angle), "x", vertical_angle)
    return None


def high_loss_clusters(grid, max_clusters=256, extra=()):
    """`grid_dbscan(grid, 0.0, 5, 10)` and ONE device-to-host copy of {total, n_clusters, table} (and of the device tensors of `extra`, which
    travel in the same copy) -> (total, count, sum_row, sum_col, the arrays of extra).  More clusters than table rows: once more with enough rows."""
    while True:
        g = grid_dbscan(grid, 0.0, HIGH_LOSS_EPS, HIGH_LOSS_MIN_SAMPLES, max_clusters=max_clusters)
        tot, n, count, sr, sc, *rest = _one_copy([g.total.reshape(1), g.n_clusters.reshape(1), g.count, g.sum_row, g.sum_col, *extra])
        if int(n[0]) <= max_clusters:
            break
        max_clusters = int(n[0])
    m = int(n[0])
    return float(tot[0]), count[:m], sr[:m], sc[:m], rest


@torch.no_grad()
def high_loss_target(view_c2w, render_depth, opacity, gt_depth, cluster_invisibility_threshold=25, hfov=90, vfov=90, max_clusters=256):
    """`get_high_loss_samples` behind its render -> (high_loss_samples_pose_c2w or None, mask_full, grid): `high_loss_grid`, DBSCAN(eps=5,
    min_samples=10) on the grid's ones, one device-to-host copy of the grid's sum and the cluster table, and the pose turned towards the centre
    of the largest cluster over `cluster_invisibility_threshold` pixels (the lowest cluster number wins a tie; None inside the 5-degree centre,
    for at most 20 ones, and without such a cluster)."""
    mask_full, grid = high_loss_grid(render_depth, opacity, gt_depth, hfov, vfov)
    total, count, sr, sc, _ = high_loss_clusters(grid, max_clusters)
    return target_from_high_loss_clusters(view_c2w, total, count, sr, sc, cluster_invisibility_threshold, hfov, vfov), mask_full, grid
