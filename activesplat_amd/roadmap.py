"""The planner's roadmap on the device: traversable map, clearance field, Voronoi skeleton, candidate nodes and the paths to them.

The stage between `topdown.topdown_maps` and `visibility.global_invisibility_scores`.  The reference builds its "Voronoi nodes" on the host every
planning step (src/planner/planner.py:111-370: cv2 contours, `scipy.spatial.Voronoi` of sampled contour points, networkx Dijkstra).  That chain
cannot be restated bit for bit (the Voronoi call perturbs its input at random), so this is a GRID FORMULATION of the same idea -- a medial axis of
free space, candidate nodes on it, shortest paths along it -- in exact integers, the same bytes every run (include/gsplat_hip.h states every rule:
gs_traversable_map .. gs_trace_path; csrc/stats.hip).  It is pinned to scipy where scipy has the operation and to numpy restatements elsewhere
(tests/roadmap_cases.py), not to the reference.  What differs from the reference on purpose:

* the reference's contour fill and `approxPolyDP` are replaced by "keep the 8-connected component that holds the agent";
* the skeleton is an integer medial axis of the pixel grid, not the Voronoi diagram of sampled contour points;
* nodes are one pick per `cell x cell` block of pixels (the skeleton pixel with the largest clearance), paths run along the skeleton.

Maps are uint8 `[H, W]` device tensors, a pixel is `(r, c)`.  `plan_roadmap` makes ONE small device-to-host copy (the node count, the entry
pixel and the status); the two geodesic fields each read 4 bytes per relaxation round.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import rasterizer as R

MAX_SIDE = 4096                        # 1 <= H, W <= 4096 (a clearance row sits in LDS; 17 H W stays below 2^31)
MAX_CELL = 64
UNREACHABLE = 2 ** 31 - 1              # what a geodesic field holds where no path arrives
STRAIGHT, DIAGONAL = 12, 17            # step weights of the geodesic fields
STATUS_AGENT_OFF_MAP = 1               # the agent's pixel is not traversable: everything is empty
STATUS_SEED_OFF_MASK = 2               # field A's seed (the agent) is outside the traversable map
STATUS_NO_ENTRY = 4                    # no roadmap pixel can be reached from the agent: field B is all unreachable, there are no nodes


def _map(t, name, dtype=torch.uint8, shape=None, tail=()):
    """a contiguous [H, W, *tail] device tensor of `dtype`, or an error that names the argument -> (tensor, H, W)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    R._require_rocm(t.device)
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() != 2 + len(tail) or tuple(t.shape[2:]) != tuple(tail) or (shape is not None and tuple(t.shape[:2]) != tuple(shape)):
        want = list(shape if shape is not None else ("H", "W")) + list(tail)
        raise ValueError(f"{name} must have shape {want}, got {list(t.shape)}")
    H, W = int(t.shape[0]), int(t.shape[1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{name}: map size {H} x {W} out of range (1 <= H, W <= {MAX_SIDE})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.detach(), H, W


def _same_device(ref, *others):
    for t, name in others:
        if t.device != ref.device:
            raise ValueError(f"{name} must be on {ref.device}, got {t.device}")


def _scratch(H, W, device, scratch=None):
    """the caller's scratch when it is large enough, else a fresh one (the caller keeps it in a name for as long as the call uses its pointer)"""
    need = int(_lib.get().gs_roadmap_scratch_bytes(H, W))
    if scratch is not None and scratch.numel() >= need and scratch.device == device:
        return scratch
    return torch.empty(need, dtype=torch.uint8, device=device)


def _rc(rc, name):
    r, c = (int(v) for v in rc)
    return r, c


@torch.no_grad()
def traversable_map(free, unseen, agent_rc, open_size=4, dilate=3, status=None, scratch=None):
    """`free`, `unseen`: `TopdownMaps.free_map_binary` and `.visible_map_binary` (1 = never seen).  m0 = free and seen; opened by an
    `open_size` square (the union of all squares inside the image and m0: the reference's 4 x 4 MORPH_OPEN); dilated by a centred `dilate`
    window clipped to the image (its 3 x 3 dilate); then the 8-connected component that holds the agent's pixel is kept -- this component rule
    deliberately replaces the reference's contour fill and approxPolyDP.  If the agent's pixel is not set the map is empty and bit 0
    (STATUS_AGENT_OFF_MAP) of `status` (a device int32 word, OR-ed into; None: dropped) is raised.  -> uint8 [H, W]"""
    free, H, W = _map(free, "free")
    unseen, _, _ = _map(unseen, "unseen", shape=(H, W))
    _same_device(free, (unseen, "unseen"))
    r, c = _rc(agent_rc, "agent_rc")
    if not (0 <= r < H and 0 <= c < W):
        raise ValueError(f"agent_rc {(r, c)} lies outside the {H} x {W} map")
    open_size, dilate = int(open_size), int(dilate)
    if not 1 <= open_size <= 16:
        raise ValueError(f"open_size must be 1..16, got {open_size}")
    if dilate % 2 != 1 or not 1 <= dilate <= 15:
        raise ValueError(f"dilate must be odd, 1..15, got {dilate}")
    dev = free.device
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    trav = torch.empty(H, W, dtype=torch.uint8, device=dev)
    scratch = _scratch(H, W, dev, scratch)
    _lib.check(_lib.get().gs_traversable_map(H, W, R._ptr(free), R._ptr(unseen), r, c, open_size, dilate, R._ptr(trav), R._ptr(scratch),
                                             R._ptr(status), _lib.stream_ptr(dev)))
    return trav


@torch.no_grad()
def clearance_field(trav, scratch=None):
    """Obstacles: the pixels with trav == 0 plus a one-pixel frame around the image.  -> (dist2 int32 [H, W]: squared distance to the nearest
    obstacle, 0 on obstacles; feature int16 [H, W, 2]: that obstacle (r, c), the lexicographically smallest among equidistant ones)"""
    trav, H, W = _map(trav, "trav")
    dev = trav.device
    dist2 = torch.empty(H, W, dtype=torch.int32, device=dev)
    feature = torch.empty(H, W, 2, dtype=torch.int16, device=dev)
    scratch = _scratch(H, W, dev, scratch)
    _lib.check(_lib.get().gs_clearance_field(H, W, R._ptr(trav), R._ptr(dist2), R._ptr(feature), R._ptr(scratch), _lib.stream_ptr(dev)))
    return dist2, feature


@torch.no_grad()
def voronoi_roadmap(trav, dist2, feature, min_dist2, gamma2=4):
    """The integer medial axis of the traversable map: for 4-adjacent traversable pixels p, q whose features lie more than sqrt(gamma2)
    apart, the one(s) nearer the bisector of the two features (ap = |p + q - 2 f(p)|^2 against aq) are marked; kept where
    dist2 >= min_dist2 = ceil(radius_px^2).  -> uint8 [H, W]"""
    trav, H, W = _map(trav, "trav")
    dist2, _, _ = _map(dist2, "dist2", torch.int32, (H, W))
    feature, _, _ = _map(feature, "feature", torch.int16, (H, W), (2,))
    _same_device(trav, (dist2, "dist2"), (feature, "feature"))
    min_dist2, gamma2 = int(min_dist2), int(gamma2)
    if min_dist2 < 0 or gamma2 < 0 or max(min_dist2, gamma2) >= 2 ** 31:
        raise ValueError("min_dist2 and gamma2 must be in 0 .. 2^31 - 1")
    out = torch.empty(H, W, dtype=torch.uint8, device=trav.device)
    _lib.check(_lib.get().gs_voronoi_roadmap(H, W, R._ptr(trav), R._ptr(dist2), R._ptr(feature), min_dist2, gamma2, R._ptr(out), _lib.stream_ptr(trav.device)))
    return out


def _geodesic(mask, H, W, seed_rc, d_seed_rc, status, scratch):
    dev = mask.device
    field = torch.empty(H, W, dtype=torch.int32, device=dev)
    rounds = C.c_int32(0)
    r, c = seed_rc
    scratch = _scratch(H, W, dev, scratch)
    _lib.check(_lib.get().gs_grid_geodesic(H, W, R._ptr(mask), r, c, R._ptr(d_seed_rc), R._ptr(field), R._ptr(scratch), R._ptr(status),
                                           C.byref(rounds), _lib.stream_ptr(dev)))
    return field, int(rounds.value)


@torch.no_grad()
def grid_geodesic(mask, seed_rc, status=None, scratch=None, return_rounds=False):
    """Shortest path lengths from `seed_rc` over the 8-connected pixels of `mask` (straight step 12, diagonal step 17; a diagonal needs only
    its two end pixels): int32 [H, W], UNREACHABLE where no path arrives.  A seed outside the mask gives an all-unreachable field and raises
    bit 1 (STATUS_SEED_OFF_MASK) of `status`.  The call reads 4 bytes per relaxation round: it waits for the device.
    return_rounds: -> (field, rounds that changed something)"""
    mask, H, W = _map(mask, "mask")
    r, c = _rc(seed_rc, "seed_rc")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=mask.device)
    field, rounds = _geodesic(mask, H, W, (r, c), None, status, scratch)
    return (field, rounds) if return_rounds else field


@torch.no_grad()
def roadmap_nodes(roadmap, dist2, field, cell, scratch=None):
    """One node per `cell x cell` block of pixels (anchored at (0, 0)): its roadmap pixel with a finite `field` and the largest `dist2`, the
    smallest index on a tie; row-major cell order.  -> (node_rc int32 [cap, 2], node_dist2 [cap], node_field [cap], count: int32 [1] on the
    DEVICE); only the first `count` rows are written (cap = the number of cells) -- `plan_roadmap` slices them after its one copy."""
    roadmap, H, W = _map(roadmap, "roadmap")
    dist2, _, _ = _map(dist2, "dist2", torch.int32, (H, W))
    field, _, _ = _map(field, "field", torch.int32, (H, W))
    _same_device(roadmap, (dist2, "dist2"), (field, "field"))
    cell = int(cell)
    if not 1 <= cell <= MAX_CELL:
        raise ValueError(f"cell must be 1..{MAX_CELL}, got {cell}")
    dev = roadmap.device
    cap = -(-H // cell) * -(-W // cell)
    node_rc = torch.zeros(cap, 2, dtype=torch.int32, device=dev)
    node_dist2 = torch.zeros(cap, dtype=torch.int32, device=dev)
    node_field = torch.zeros(cap, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(H, W, dev, scratch)
    _lib.check(_lib.get().gs_roadmap_nodes(H, W, R._ptr(roadmap), R._ptr(dist2), R._ptr(field), cell, R._ptr(node_rc), R._ptr(node_dist2), R._ptr(node_field),
                                           R._ptr(count), R._ptr(scratch), _lib.stream_ptr(dev)))
    return node_rc, node_dist2, node_field, count


@torch.no_grad()
def trace_path(mask, field, target_rc, capacity, return_status=False):
    """Walk down `field` from the target to its seed: step to the first neighbour n in the mask, in the order (-1,-1), (-1,0), (-1,1), (0,-1),
    (0,1), (1,-1), (1,0), (1,1), with field[n] + w == field[current]; stop where the field reads 0.  One wavefront walks; `capacity` bounds
    it.  `target_rc`: two ints, or a DEVICE int32 pair.  -> (path int32 [capacity, 2] on the device, count2: device int32 [2] = pixels written,
    0 done | 1 target off the mask or unreachable | 2 capacity reached | 3 not a field of this mask); with return_status the pair is copied
    (which waits) -> (path[:n], status)"""
    mask, H, W = _map(mask, "mask")
    field, _, _ = _map(field, "field", torch.int32, (H, W))
    _same_device(mask, (field, "field"))
    capacity = int(capacity)
    if capacity < 0 or capacity >= 2 ** 30:
        raise ValueError(f"capacity must be 0 .. 2^30 - 1, got {capacity}")
    dev = mask.device
    d_target, r, c = None, -1, -1
    if torch.is_tensor(target_rc):
        if target_rc.dtype != torch.int32 or target_rc.numel() != 2 or not target_rc.is_contiguous() or target_rc.device != dev:
            raise ValueError("a tensor target_rc must be a contiguous int32 pair on the mask's device")
        d_target = target_rc
    else:
        r, c = _rc(target_rc, "target_rc")
    path = torch.zeros(max(capacity, 1), 2, dtype=torch.int32, device=dev)
    count2 = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.check(_lib.get().gs_trace_path(H, W, R._ptr(mask), R._ptr(field), r, c, R._ptr(d_target), capacity, R._ptr(path), R._ptr(count2), _lib.stream_ptr(dev)))
    if not return_status:
        return path, count2
    n, st = (int(v) for v in count2.tolist())
    return path[:n], st


class Roadmap:
    """What `plan_roadmap` found.  Device tensors: `trav`, `roadmap` uint8 [H, W]; `dist2` int32 [H, W], `feature` int16 [H, W, 2];
    `field_agent` (A: over the traversable map from the agent) and `field_entry` (B: over the roadmap from the entry) int32 [H, W];
    `node_rc` int32 [K, 2], `node_dist2`, `node_field` (field B at the node) [K].  Host values: `K`, `agent_rc`, `entry_rc` ((-1, -1) when no
    roadmap pixel can be reached), `entry_field` (field A at the entry), `status` (STATUS_* bits), `rounds` (relaxation rounds of A and B)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def path_capacity(self):
        return int(self.trav.shape[0]) * int(self.trav.shape[1])

    @torch.no_grad()
    def path_to(self, node):
        """Pixels from the agent to node `node` (0 <= node < K), both included: the trace down field B (node -> entry) followed by the trace
        down field A (entry -> agent), reversed into agent-to-node order; the entry pixel appears once.  -> path int32 [n, 2] on the device;
        its length in the fields' weights is `node_path_length()[node]`.  One 16-byte copy of the two counts (which waits for the device).
        Raises when a trace fails (it cannot: nodes are picked among the pixels with a finite field B)."""
        node = int(node)
        if not 0 <= node < self.K:
            raise IndexError(f"node {node} out of range (K = {self.K})")
        cap = self.path_capacity
        pb, cb = trace_path(self.roadmap, self.field_entry, self.node_rc[node], cap)
        pa, ca = trace_path(self.trav, self.field_agent, self.entry_rc, cap)
        nb, sb, na, sa = (int(v) for v in torch.cat([cb, ca]).tolist())
        if sb or sa:
            raise RuntimeError(f"path_to({node}): trace status {sb} on the roadmap, {sa} on the traversable map")
        return torch.cat([pb[:nb], pa[1:na]]).flip(0).contiguous()

    def node_path_length(self):
        """field A at the entry + field B at each node: int64 [K] on the device (the length of `path_to`'s path in the fields' weights)"""
        return self.node_field.to(torch.int64) + int(self.entry_field)


@torch.no_grad()
def plan_roadmap(maps, agent_rc, radius_px, cell, open_size=4, dilate=3, gamma2=4):
    """`maps`: a `topdown.TopdownMaps` (or any object with `free_map_binary` and `visible_map_binary`); `agent_rc`: the agent's pixel;
    `radius_px`: the agent's radius in pixels (roadmap pixels keep dist2 >= ceil(radius_px^2)); `cell`: the node spacing in pixels.
    traversable map -> clearance field -> roadmap -> field A over the traversable map from the agent -> entry = the roadmap pixel with the
    smallest field A (smallest index on a tie) -> field B over the roadmap from the entry -> nodes -> ONE device-to-host copy of K, the entry
    and the status.  -> Roadmap"""
    free, unseen = maps.free_map_binary, maps.visible_map_binary
    free, H, W = _map(free, "free_map_binary")
    radius_px = float(radius_px)
    if not (0.0 <= radius_px < math.inf):
        raise ValueError("radius_px must be finite and not negative")
    min_dist2 = int(math.ceil(radius_px * radius_px))
    lib, dev = _lib.get(), free.device
    scratch = _scratch(H, W, dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)               # [traversable | field A | field B | spare]
    agent = _rc(agent_rc, "agent_rc")
    trav = traversable_map(free, unseen, agent, open_size, dilate, status[0:1], scratch)
    dist2, feature = clearance_field(trav, scratch)
    roadmap = voronoi_roadmap(trav, dist2, feature, min_dist2, gamma2)
    field_a, rounds_a = _geodesic(trav, H, W, agent, None, status[1:2], scratch)
    entry = torch.empty(4, dtype=torch.int32, device=dev)
    _lib.check(lib.gs_roadmap_entry(H, W, R._ptr(roadmap), R._ptr(field_a), R._ptr(entry), R._ptr(scratch), _lib.stream_ptr(dev)))
    field_b, rounds_b = _geodesic(roadmap, H, W, (-1, -1), entry, status[2:3], scratch)
    node_rc, node_dist2, node_field, count = roadmap_nodes(roadmap, dist2, field_b, cell, scratch)
    K, er, ec, ef, _, s0, s1, s2, _ = (int(v) for v in torch.cat([count, entry, status]).tolist())       # the one copy
    return Roadmap(trav=trav, dist2=dist2, feature=feature, roadmap=roadmap, field_agent=field_a, field_entry=field_b,
                   node_rc=node_rc[:K], node_dist2=node_dist2[:K], node_field=node_field[:K], K=K, agent_rc=agent, entry_rc=(er, ec), entry_field=ef,
                   status=(s0 & 1) | (STATUS_SEED_OFF_MASK if s1 & 2 else 0) | (STATUS_NO_ENTRY if s2 & 2 else 0), rounds=(rounds_a, rounds_b),
                   cell=int(cell), min_dist2=min_dist2)


# ---- subregions, line tests --------------------------------------------------------------------------------------------------------------------
# What the reference's hierarchical target choice (scripts/nodes/planner_node.py:249-463, activesplat_amd/policy.py) needs on top of a Roadmap:
# the all-pairs node distances, the clustering of the nodes into subregions (src/planner/planner.py:530-574) and the line tests of
# planner.py:473-528 and planner_node.py:1173-1200, here on the clearance field.  The rules: include/gsplat_hip.h, gs_node_distances ..
# gs_subregions.  The calls enqueue work and wait for nothing; there is no CPU fallback.

MAX_NODES = 1024                       # GS_MAX_NODES: the node count gs_node_distances and gs_subregions take
NODE_DISTANCE_PATHS = {"auto": 0, "lds": 1, "global": 2}


def set_node_distance_path(path):
    """test knob: where `node_distances` keeps a seed's distances -- "lds" (only where the skeleton fits), "global", or "auto" by size"""
    _lib.check(_lib.get().gs_set_node_distance_path(NODE_DISTANCE_PATHS[path]))


def _nodes(node_rc, device, name="node_rc"):
    if not torch.is_tensor(node_rc):
        raise TypeError(f"{name} must be a torch tensor, got {type(node_rc).__name__}")
    if node_rc.dtype != torch.int32 or node_rc.dim() != 2 or node_rc.shape[1] != 2 or not node_rc.is_contiguous() or node_rc.device != device:
        raise ValueError(f"{name} must be a contiguous int32 [K, 2] tensor on {device}")
    K = int(node_rc.shape[0])
    if K > MAX_NODES:
        raise ValueError(f"{name}: {K} nodes, at most {MAX_NODES} are taken")
    return node_rc.detach(), K


@torch.no_grad()
def node_distances(rm, node_rc=None, scratch=None):
    """D int32 [K, K] on the device: D[i][j] = the shortest path length from node i to node j along the roadmap, in `grid_geodesic`'s weights
    (exactly `grid_geodesic(rm.roadmap, node_rc[i])[node_rc[j]]`: symmetric, 0 on the diagonal, UNREACHABLE where no path exists).  One call:
    no per-seed host loop, nothing is read back.  `rm`: a Roadmap, or a uint8 [H, W] mask together with `node_rc` (int32 [K, 2] on the device;
    default: the Roadmap's nodes).  K <= MAX_NODES."""
    mask = rm.roadmap if isinstance(rm, Roadmap) else rm
    mask, H, W = _map(mask, "roadmap")
    node_rc, K = _nodes(rm.node_rc if node_rc is None else node_rc, mask.device)
    lib, dev = _lib.get(), mask.device
    need = int(lib.gs_node_distances_scratch_bytes(H, W))
    if scratch is None or scratch.numel() < need or scratch.device != dev:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    D = torch.empty(K, K, dtype=torch.int32, device=dev)
    _lib.check(lib.gs_node_distances(H, W, R._ptr(mask), K, R._ptr(node_rc) if K else None, R._ptr(D) if K else None, R._ptr(scratch), _lib.stream_ptr(dev)))
    return D


@torch.no_grad()
def segment_clearance(dist2, segments):
    """`segments`: int32 [n, 4] = (r0, c0, r1, c1) on the device, end points outside the image allowed.  -> int32 [n]: the minimum of `dist2`
    over the pixels of the integer line (pixel i of N = max(|dr|, |dc|) is (r0 + floor((2 i dr + N) / (2 N)), c0 + likewise)); a pixel outside
    the image counts as an obstacle (0).  A segment is clear for a radius rho when its clearance >= ceil(rho^2)."""
    dist2, H, W = _map(dist2, "dist2", torch.int32)
    if not torch.is_tensor(segments):
        raise TypeError(f"segments must be a torch tensor, got {type(segments).__name__}")
    if segments.dtype != torch.int32 or segments.dim() != 2 or segments.shape[1] != 4 or not segments.is_contiguous() or segments.device != dist2.device:
        raise ValueError(f"segments must be a contiguous int32 [n, 4] tensor on {dist2.device}")
    n = int(segments.shape[0])
    out = torch.empty(n, dtype=torch.int32, device=dist2.device)
    _lib.check(_lib.get().gs_segment_clearance(H, W, R._ptr(dist2), n, R._ptr(segments) if n else None, R._ptr(out) if n else None,
                                               _lib.stream_ptr(dist2.device)))
    return out


def _from_agent(rm, rc):
    """segments agent -> each of `rc` (int32 [n, 2] on the device)"""
    agent = torch.tensor(rm.agent_rc, dtype=torch.int32, device=rc.device).expand(rc.shape[0], 2)          # (the one small copy: 8 bytes up)
    return torch.cat([agent, rc], 1).contiguous()


@torch.no_grad()
def nodes_in_horizon(rm):
    """uint8 [K] on the device: 1 where the integer line from the agent's pixel to the node runs wholly on `rm.trav` (its clearance >= 1).
    The reference's IN_HORIZON flag (planner_node.py:1173-1200) is a 1-pixel `cv2.line` on its free map, with the agent's own disc masked
    out of the test; this is the grid rule of `segment_clearance` instead, and the agent's disc is NOT masked out."""
    return (segment_clearance(rm.dist2, _from_agent(rm, rm.node_rc)) >= 1).to(torch.uint8)


def path_length_px(path_rc):
    """the Euclidean sum over the vertices of a pixel path [n, 2], in fp64 on the device -> 0-dim tensor"""
    d = (path_rc[1:] - path_rc[:-1]).to(torch.float64)
    return torch.sqrt((d * d).sum(1)).sum()


@torch.no_grad()
def shortcut_path(rm, path_rc, radius_px, ratio=1.5):
    """The reference's "fast forward" and safe-path tests (planner.py:473-528) on the clearance field.  `path_rc`: the agent-to-node pixel
    path of `rm.path_to` (int32 [n, 2], n >= 1, its first pixel the agent's).  k = the LARGEST index whose segment from the agent is clear for
    the radius `ratio * radius_px` (clearance >= ceil((ratio radius_px)^2); k = 0, the agent's own pixel, always qualifies).  The reference
    walks back from the far end and also stops early once the distance to the agent starts to grow again; that early break is deliberately
    dropped.  -> (path int32 [n - k + 1, 2]: the agent's pixel followed by path_rc[k:], k: 0-dim int64, safe: 0-dim uint8 -- the clearance of
    the agent -> path_rc[k] segment >= ceil(radius_px^2); the pixels behind it are roadmap pixels (or the traversable way to the entry)
    and keep dist2 >= min_dist2), all on the device.  One 8-byte copy (k sizes the result)."""
    if not torch.is_tensor(path_rc) or path_rc.dtype != torch.int32 or path_rc.dim() != 2 or path_rc.shape[1] != 2 or path_rc.shape[0] < 1:
        raise ValueError("path_rc must be an int32 [n, 2] tensor with n >= 1")
    radius_px, ratio = float(radius_px), float(ratio)
    if not (0.0 <= radius_px < math.inf and 0.0 <= ratio < math.inf):
        raise ValueError("radius_px and ratio must be finite and not negative")
    path_rc = path_rc.contiguous()
    clear = segment_clearance(rm.dist2, _from_agent(rm, path_rc))
    ok = clear >= int(math.ceil((ratio * radius_px) ** 2))
    ok[0] = True
    index = torch.arange(path_rc.shape[0], device=path_rc.device)
    k = torch.where(ok, index, torch.zeros_like(index)).max()
    safe = (clear[k] >= int(math.ceil(radius_px * radius_px))).to(torch.uint8)
    agent = torch.tensor([rm.agent_rc], dtype=torch.int32, device=path_rc.device)
    return torch.cat([agent, path_rc[int(k.item()):]]), k, safe


@torch.no_grad()
def subregions(rm, D, px_per_m, path_weight=0.5, coord_weight=0.5, scope_m=2.0, node_rc=None, scratch=None):
    """The reference's `get_subregions` (planner.py:530-574) on the device, in fp64: C[i][j] = path_weight D[i][j] / 12 + coord_weight
    |node_i - node_j| (pixels; the largest finite C + 1 where D is UNREACHABLE), average linkage -- merge the two clusters with the smallest
    average pairwise C, on a tie the pair whose smallest members are lexicographically smallest -- until that minimum exceeds
    scope_m * px_per_m: `fcluster(linkage(C, 'average'), t, 'distance')`.  `rm`: a Roadmap (or None with `node_rc` given).
    -> (labels int32 [K]: clusters numbered 0, 1, .. by their smallest member; count int32 [1]; heights fp64 [K - 1]: the merge heights in
    merge order, +inf from the first merge not made), all on the device."""
    if not torch.is_tensor(D):
        raise TypeError(f"D must be a torch tensor, got {type(D).__name__}")
    node_rc, K = _nodes(rm.node_rc if node_rc is None else node_rc, D.device)
    if D.dtype != torch.int32 or tuple(D.shape) != (K, K) or not D.is_contiguous():
        raise ValueError(f"D must be a contiguous int32 [{K}, {K}] tensor, got {D.dtype} {list(D.shape)}")
    R._require_rocm(D.device)
    t = float(scope_m) * float(px_per_m)
    path_weight, coord_weight = float(path_weight), float(coord_weight)
    if not (0.0 <= path_weight < math.inf and 0.0 <= coord_weight < math.inf and t >= 0.0):
        raise ValueError("path_weight and coord_weight must be finite and not negative, scope_m * px_per_m not negative")
    lib, dev = _lib.get(), D.device
    need = int(lib.gs_subregions_scratch_bytes(K))
    if scratch is None or scratch.numel() < need or scratch.device != dev:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    labels = torch.empty(K, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    heights = torch.empty(max(K - 1, 0), dtype=torch.float64, device=dev)
    _lib.check(lib.gs_subregions(K, R._ptr(node_rc) if K else None, R._ptr(D) if K else None, path_weight, coord_weight, t, R._ptr(labels) if K else None,
                                 R._ptr(count), R._ptr(heights) if K > 1 else None, R._ptr(scratch), _lib.stream_ptr(dev)))
    return labels, count, heights


# ---- pixels and the world ------------------------------------------------------------------------------------------------------------------------
# `topdown.topdown_camera` looks down the +y axis from `height` metres above `world_center` = (x, z): camera x = world x, camera y = -world z,
# depth = world y + height, fx = W height / world_width, fy = H height / world_height, principal point (W // 2, H // 2).  The rasteriser samples
# pixel (r, c) at the image position (c, r) = (fx X / Z + cx - 0.5, fy Y / Z + cy - 0.5) (ndc -> ((ndc + 1) S - 1) / 2).  A pixel names the ray
# through its sample position; on the plane world y = `y` (default 0, the floor of the mapper's y-down world at the camera's height) that is:

def world_to_pixel(xz, world_center, world_shape, grid_shape, height=1000.0, y=0.0):
    """host: world (x, z) [..., 2] at height `y` -> continuous (r, c) [..., 2] float64; the pixel that shows the point is `np.rint` of it"""
    xz = np.asarray(xz, dtype=np.float64)
    W, H = int(grid_shape[0]), int(grid_shape[1])
    fx, fy = W * height / float(world_shape[0]), H * height / float(world_shape[1])
    depth = float(y) + height
    c = fx * (xz[..., 0] - float(world_center[0])) / depth + (W // 2) - 0.5
    r = fy * -(xz[..., 1] - float(world_center[1])) / depth + (H // 2) - 0.5
    return np.stack([r, c], -1)


def pixel_to_world(rc, world_center, world_shape, grid_shape, height=1000.0, y=0.0):
    """the inverse of `world_to_pixel`: pixel (r, c) [..., 2] (host array, or a device tensor: the result is a float32 tensor on its device)
    -> world (x, z) [..., 2] of the pixel's sample position on the plane world y = `y`"""
    W, H = int(grid_shape[0]), int(grid_shape[1])
    fx, fy = W * height / float(world_shape[0]), H * height / float(world_shape[1])
    depth = float(y) + height
    if torch.is_tensor(rc):
        rcf = rc.to(torch.float64)
        x = (rcf[..., 1] + 0.5 - (W // 2)) * depth / fx + float(world_center[0])
        z = -(rcf[..., 0] + 0.5 - (H // 2)) * depth / fy + float(world_center[1])
        return torch.stack([x, z], -1).to(torch.float32)
    rc = np.asarray(rc, dtype=np.float64)
    x = (rc[..., 1] + 0.5 - (W // 2)) * depth / fx + float(world_center[0])
    z = -(rc[..., 0] + 0.5 - (H // 2)) * depth / fy + float(world_center[1])
    return np.stack([x, z], -1)
