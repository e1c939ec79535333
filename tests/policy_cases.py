"""Shared checks of the roadmap subregions and the hierarchical target choice (activesplat_amd/roadmap.py: node_distances, segment_clearance,
nodes_in_horizon, shortcut_path, subregions; activesplat_amd/policy.py; gs_node_distances, gs_segment_clearance, gs_subregions): run on the
host-emulated kernels by tests/test_policy.py and on the MI355X by tests/test_gpu_policy.py, every device check inside
guard.guarded_allocations.  The maps and their references are those of tests/roadmap_cases.py.

Expected values, none of them from the code under test:
* node distances     scipy.sparse.csgraph.dijkstra on the roadmap mask's 12 / 17 graph from every node, sampled at the nodes: exact equality;
* segment clearance  `ref_line` / `ref_clearance`, the line rule of include/gsplat_hip.h in Python integers: exact equality;
* subregions         (a) `ref_linkage`, the stated rule in numpy fp64 (labels exact, heights to 1e-12 relative); (b) scipy's
                     fcluster(linkage(squareform(C), 'average'), t, 'distance'), relabelled canonically; (c) the labels the reference's
                     get_subregions returned (tests/golden/subregions.npz, written by tests/golden/make_subregions_golden.py);
* policy             `ref_scores`, a restatement of planner_node.py:1201-1215, and hand-made scenarios, one per branch of `choose`.
"""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch
from scipy.cluster import hierarchy as hc
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra
from scipy.spatial.distance import squareform

from activesplat_amd import _lib
from activesplat_amd import policy as PL
from activesplat_amd import rasterizer as R
from activesplat_amd import roadmap as RM
from tests import roadmap_cases as rc
from tests.roadmap_cases import guarded, n, t

GS_EINVAL = 1
INF = RM.UNREACHABLE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subregions.npz")


# ---- node distances ------------------------------------------------------------------------------------------------------------------------------

def mask_graph(mask):
    """the 8-connected pixels of the mask as a csr graph, straight step 12, diagonal step 17 (a diagonal needs only its two end pixels)"""
    H, W = mask.shape
    m = mask != 0
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, w = [], [], []
    for dr, dc in rc.STEPS:
        a = (slice(max(0, -dr), H - max(0, dr)), slice(max(0, -dc), W - max(0, dc)))
        b = (slice(max(0, dr), H - max(0, -dr)), slice(max(0, dc), W - max(0, -dc)))
        ok = m[a] & m[b]
        rows.append(idx[a][ok]); cols.append(idx[b][ok]); w.append(np.full(int(ok.sum()), 17.0 if dr and dc else 12.0))
    return coo_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()


def ref_node_distances(mask, node_rc):
    """scipy's Dijkstra from every node, sampled at the nodes (exact in float64) -> int32 [K, K]; a node outside the image or off the mask has
    INF in its whole row and column, as the geodesic field seeded there has"""
    H, W = mask.shape
    node_rc = np.asarray(node_rc, np.int64).reshape(-1, 2)
    K = len(node_rc)
    D = np.full((K, K), INF, np.int32)
    on = np.array([0 <= r < H and 0 <= c < W and mask[r, c] != 0 for r, c in node_rc], bool)
    if on.any():
        p = node_rc[on, 0] * W + node_rc[on, 1]
        d = dijkstra(mask_graph(mask), directed=True, indices=p)[:, p]
        sub = np.where(np.isfinite(d), d, INF).astype(np.int32)
        D[np.ix_(on, on)] = sub
    return D


def run_node_distances(device, mask, node_rc):
    D = RM.node_distances(t(mask, device), t(np.asarray(node_rc, np.int32).reshape(-1, 2), device))
    assert D.dtype == torch.int32
    return n(D)


@guarded
def check_node_distances_case(device, name):
    """a case of roadmap_cases: D through the Roadmap of plan_roadmap against scipy at the reference's nodes"""
    cs, ref = rc.case(name), rc.reference(name)
    want = ref_node_distances(ref.roadmap, ref.node_rc)
    maps = types.SimpleNamespace(free_map_binary=t(cs.free, device), visible_map_binary=t(cs.unseen, device))
    rm = RM.plan_roadmap(maps, cs.agent, float(np.sqrt(max(0.0, cs.min_dist2 - 0.5))), cs.cell, cs.open_size, cs.dilate)
    assert np.array_equal(n(rm.node_rc), ref.node_rc)
    got = n(RM.node_distances(rm))
    assert got.shape == (rm.K, rm.K) and np.array_equal(got, want), name
    if rm.K:
        assert (got != INF).all() and np.array_equal(got, got.T) and not np.diag(got).any(), "nodes are mutually reachable"
        # row 0 is the geodesic field from node 0 sampled at the nodes
        field = n(RM.grid_geodesic(rm.roadmap, tuple(int(v) for v in ref.node_rc[0])))
        assert np.array_equal(got[0], field[ref.node_rc[:, 0], ref.node_rc[:, 1]])


@guarded
def check_node_distances_two_doors(device):
    """two routes between the two sides of the wall: the shorter one wins, in both directions"""
    ref = rc.reference("two-doors-9")
    nodes = ref.node_rc
    left, right = np.flatnonzero(nodes[:, 1] < 18), np.flatnonzero(nodes[:, 1] > 21)
    assert len(left) and len(right)
    want = ref_node_distances(ref.roadmap, nodes)
    cut = ref.roadmap.copy()
    cut[9:15, 18:22] = 0                                               # without the narrow door every crossing goes the long way
    longer = ref_node_distances(cut, nodes)
    assert (longer[np.ix_(left, right)] > want[np.ix_(left, right)]).any(), "some pair crosses by the narrow door"
    got = run_node_distances(device, ref.roadmap, nodes)
    assert np.array_equal(got, want) and np.array_equal(got, got.T)
    assert np.array_equal(run_node_distances(device, cut, nodes), longer)


@guarded
def check_node_distances_serpentine(device):
    """nodes along a 96 x 96 serpentine corridor: long paths, many relaxation sweeps"""
    mask = rc.serpentine()
    nodes = np.array([(3, 3), (3, 90), (54, 50), (92, 92), (92, 3), (13, 40)], np.int32)
    assert all(mask[r, c] for r, c in nodes)
    want = ref_node_distances(mask, nodes)
    assert (want != INF).all() and want.max() > 12 * 96 * 4
    assert np.array_equal(run_node_distances(device, mask, nodes), want)


@guarded
def check_node_distances_small(device):
    """K = 0, 1, 2 by hand-made node lists; a mask with two components; a node pixel given twice; nodes off the mask and outside the image"""
    ref = rc.reference("48x40")
    on = np.argwhere(ref.roadmap != 0).astype(np.int32)
    assert run_node_distances(device, ref.roadmap, np.zeros((0, 2), np.int32)).shape == (0, 0)
    assert np.array_equal(run_node_distances(device, ref.roadmap, on[:1]), [[0]])
    for nodes in (on[[0, -1]], on[[3, 3, len(on) // 2]], np.array([on[0], (0, 0), on[-1], (-1, 5), (5, 40)], np.int32)):
        want = ref_node_distances(ref.roadmap, nodes)
        assert np.array_equal(run_node_distances(device, ref.roadmap, nodes), want)
    twice = ref_node_distances(ref.roadmap, on[[3, 3, len(on) // 2]])
    assert twice[0, 1] == 0 and twice[1, 0] == 0, "one pixel given twice: D = 0 off the diagonal"
    ref17 = rc.reference("two-doors-17")                               # the roadmap is cut at both doors: two components
    nodes, _, _ = rc.ref_nodes(ref17.roadmap, ref17.dist2, np.zeros_like(ref17.field_b), 8)
    want = ref_node_distances(ref17.roadmap, nodes)
    assert (want == INF).any() and (want != INF).any() and np.array_equal(want, want.T)
    assert np.array_equal(run_node_distances(device, ref17.roadmap, nodes), want)
    # an all-clear mask: no skeleton pixel at all
    assert (run_node_distances(device, np.zeros((5, 7), np.uint8), np.array([(1, 1), (2, 2)], np.int32)) == INF).all()


@guarded
def check_node_distances_paths(device):
    """each size-selected path forced on the 48 x 40 case: the same matrix"""
    ref = rc.reference("48x40")
    want = ref_node_distances(ref.roadmap, ref.node_rc)
    try:
        for path in ("lds", "global", "auto"):
            RM.set_node_distance_path(path)
            assert np.array_equal(run_node_distances(device, ref.roadmap, ref.node_rc), want), path
    finally:
        RM.set_node_distance_path("auto")
    assert _lib.get().gs_set_node_distance_path(3) == GS_EINVAL and _lib.get().gs_set_node_distance_path(-1) == GS_EINVAL


# ---- segment clearance ---------------------------------------------------------------------------------------------------------------------------

def ref_line(r0, c0, r1, c1):
    """the pixels of the integer line one after the other, in Python integers (// is floor division)"""
    dr, dc = r1 - r0, c1 - c0
    N = max(abs(dr), abs(dc))
    if N == 0:
        yield (r0, c0)
        return
    for i in range(N + 1):
        yield (r0 + (2 * i * dr + N) // (2 * N), c0 + (2 * i * dc + N) // (2 * N))


def ref_clearance(dist2, segments):
    """the minimum over the line; dist2 is never negative, so the walk ends at the first 0 (a pixel outside the image is one)"""
    H, W = dist2.shape
    out = []
    for r0, c0, r1, c1 in np.asarray(segments, np.int64).tolist():
        best = INF
        for r, c in ref_line(r0, c0, r1, c1):
            best = min(best, int(dist2[r, c]) if 0 <= r < H and 0 <= c < W else 0)
            if best == 0:
                break
        out.append(best)
    return np.array(out, np.int32)


def segment_set(H, W, seed=0):
    """random segments inside the image, the eight octants, N = 0, the axes and the diagonals, lines whose rounding hits the exact half
    (N even, i * d odd: d odd; both signs), end points outside the image on each side (near and far)"""
    rng = np.random.RandomState(seed)
    segs = [tuple(int(v) for v in (rng.randint(H), rng.randint(W), rng.randint(H), rng.randint(W))) for _ in range(150)]
    r, c = H // 2, W // 2
    segs += [(r, c, r + dr, c + dc) for dr, dc in ((3, 11), (11, 3), (-3, 11), (-11, 3), (3, -11), (11, -3), (-3, -11), (-11, -3))]     # octants
    segs += [(r, c, r, c), (0, 0, 0, 0), (H - 1, W - 1, H - 1, W - 1)]                                                                    # N = 0
    segs += [(r, 1, r, W - 2), (r, W - 2, r, 1), (1, c, H - 2, c), (H - 2, c, 1, c)]                                                       # axes
    segs += [(r, c, r + 9, c + 9), (r, c, r - 9, c + 9), (r, c, r + 9, c - 9), (r, c, r - 9, c - 9)]                                       # slope +-1
    segs += [(r, c, r + dr, c + dc) for dr, dc in ((12, 5), (12, -5), (-12, 5), (-12, -5), (5, 12), (-5, 12), (5, -12), (-5, -12), (2, 1), (-2, -1),
                                                    (1, -2), (-1, 2), (10, 7), (-10, -7), (7, -10), (-7, 10))]                              # halves
    segs += [(r, c, -1, c), (r, c, H, c), (r, c, r, -1), (r, c, r, W), (-3, -3, r, c), (r, c, H + 5, W + 7), (r, c, r, 10 ** 6),
             (-2 ** 31, 0, 2 ** 31 - 1, 0), (r, c, -10 ** 9, 10 ** 9), (-5, 2, -1, 8)]                                                     # outside
    return np.array(segs, np.int64).astype(np.int32)


def check_line_rule():
    """the restatement itself: end points, steps of at most one pixel, the half rounds towards +infinity for both signs"""
    line = lambda *s: list(ref_line(*s))
    assert line(0, 0, 2, 1) == [(0, 0), (1, 1), (2, 1)] and line(0, 0, -2, -1) == [(0, 0), (-1, 0), (-2, -1)]
    assert line(5, 5, 5, 5) == [(5, 5)] and line(0, 0, 0, 3) == [(0, 0), (0, 1), (0, 2), (0, 3)]
    for s in segment_set(48, 40)[:190].tolist():
        px = np.array(line(*s))
        assert tuple(px[0]) == tuple(s[:2]) and tuple(px[-1]) == tuple(s[2:]) and len(px) == max(abs(s[2] - s[0]), abs(s[3] - s[1])) + 1
        assert np.abs(np.diff(px, axis=0)).max(initial=0) <= 1
    halves = [s for s in segment_set(48, 40).tolist() if max(abs(s[2] - s[0]), abs(s[3] - s[1])) % 2 == 0 and min(abs(s[2] - s[0]), abs(s[3] - s[1])) % 2 == 1]
    assert len(halves) >= 8


@guarded
def check_segment_clearance(device):
    for name in ("48x40", "67x130"):
        dist2 = rc.reference(name).dist2
        segs = segment_set(*dist2.shape)
        want = ref_clearance(dist2, segs)
        assert (want > 0).sum() >= 20 and (want == 0).sum() >= 20
        got = RM.segment_clearance(t(dist2, device), t(segs, device))
        assert got.dtype == torch.int32 and np.array_equal(n(got), want), name
    assert n(RM.segment_clearance(t(dist2, device), t(np.zeros((0, 4), np.int32), device))).shape == (0,)


def two_doors_roadmap(device, min_dist2=9):
    cs = rc.case(f"two-doors-{min_dist2}")
    maps = types.SimpleNamespace(free_map_binary=t(cs.free, device), visible_map_binary=t(cs.unseen, device))
    return RM.plan_roadmap(maps, cs.agent, float(np.sqrt(cs.min_dist2 - 0.5)), cs.cell), rc.reference(f"two-doors-{min_dist2}")


@guarded
def check_horizon_and_shortcut(device):
    """two doors, the agent at (24, 8) left of the wall: a node behind the wall is out of the horizon; the shortcut of a path through a door
    stops at the door"""
    rm, ref = two_doors_roadmap(device)
    agent, nodes = rm.agent_rc, ref.node_rc
    want = np.array([min(int(ref.trav[r, c]) if 0 <= r < 48 and 0 <= c < 40 else 0 for r, c in ref_line(*agent, *node)) for node in nodes.tolist()], np.uint8)
    got = RM.nodes_in_horizon(rm)
    assert got.dtype == torch.uint8 and np.array_equal(n(got), want)
    behind = [k for k, (r, c) in enumerate(nodes.tolist()) if c > 21 and 16 <= r <= 28]                # straight across the wall from the agent
    assert behind and not want[behind].any() and want[nodes[:, 1] < 18].any(), "a node behind the wall is out of the horizon, some node is in it"
    radius = 2.0
    for k in (behind[0], int(np.flatnonzero(nodes[:, 1] < 18)[0])):
        path = n(rm.path_to(k))
        clear = ref_clearance(ref.dist2, np.concatenate([np.tile(agent, (len(path), 1)), path], 1))
        ok = clear >= math.ceil((1.5 * radius) ** 2)
        ok[0] = True
        kk = int(np.flatnonzero(ok).max())
        short, k_dev, safe = RM.shortcut_path(rm, t(path, device), radius, 1.5)
        assert int(k_dev.item()) == kk and np.array_equal(n(short), np.concatenate([[agent], path[kk:]]))
        assert int(safe.item()) == int(clear[kk] >= math.ceil(radius * radius)) == 1 and safe.dtype == torch.uint8
        if k == behind[0]:
            assert 0 < kk < len(path) - 1 and path[kk][1] <= 22, "the straight line ends where the way turns through the door"
        want_len = float(np.sqrt((np.diff(n(short).astype(np.float64), axis=0) ** 2).sum(1)).sum())
        assert abs(float(RM.path_length_px(short).item()) - want_len) <= 1e-12 * max(1.0, want_len) and RM.path_length_px(short).dtype == torch.float64
    one, k0, safe0 = RM.shortcut_path(rm, t(np.array([agent], np.int32), device), radius)
    assert int(k0.item()) == 0 and np.array_equal(n(one), [agent, agent]) and int(safe0.item()) == 1


# ---- subregions ------------------------------------------------------------------------------------------------------------------------------------

def ref_C(node_rc, D, path_weight=0.5, coord_weight=0.5):
    """the clustering distance in numpy fp64: two products and one sum per pair; the largest finite entry + 1 where D is unreachable"""
    p = np.asarray(node_rc, np.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    with np.errstate(invalid="ignore"):
        C = path_weight * (D.astype(np.float64) / 12.0) + coord_weight * np.sqrt(d2.astype(np.float64))
    C[D == INF] = np.inf
    np.fill_diagonal(C, 0.0)
    finite = C[np.isfinite(C)]
    C[np.isinf(C)] = (finite.max() if len(finite) else 0.0) + 1.0
    return C


def ref_linkage(C, threshold):
    """the stated rule, naively: clusters named by their smallest member, the sums per cluster pair added on a merge, the smallest average,
    ties to the lexicographically smallest (a, b) -> (canonical labels int32 [K], heights fp64 [K - 1])"""
    K = len(C)
    S, size, live = C.astype(np.float64).copy(), np.ones(K, np.int64), np.ones(K, bool)
    member, heights = np.arange(K), np.full(max(K - 1, 0), np.inf)
    for step in range(K - 1):
        ids = np.flatnonzero(live)
        avg = S[np.ix_(ids, ids)] / (size[ids][:, None] * size[ids][None, :]).astype(np.float64)
        avg[np.tril_indices(len(ids))] = np.inf
        flat = int(np.argmin(avg))                                     # the first minimum in row-major order: the smallest (a, b)
        a, b = int(ids[flat // len(ids)]), int(ids[flat % len(ids)])
        if not avg.reshape(-1)[flat] <= threshold:
            break
        heights[step] = avg.reshape(-1)[flat]
        s = S[a] + S[b]
        S[a, :] = s; S[:, a] = s
        size[a] += size[b]; live[b] = False
        member[member == b] = a
    return canonical(member), heights


def canonical(labels):
    """clusters numbered 0, 1, .. by their smallest member"""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse].astype(np.int32)


def scipy_labels(C, threshold):
    """-> (canonical labels, scipy's merge heights); a single node cannot be linked (scipy refuses an empty distance matrix): it is its own cluster"""
    if len(C) < 2:
        return np.zeros(len(C), np.int32), np.zeros(0)
    Z = hc.linkage(squareform(C, checks=False), method="average")
    return canonical(hc.fcluster(Z, t=threshold, criterion="distance")), Z[:, 2]


#: (key, the roadmap case, K, seed, px_per_m, reachable only): t = 2 m * px_per_m pixels.  The nodes are K roadmap pixels drawn with the seed, NOT the
#: roadmap's own nodes: one node per 8 x 8 cell puts many pairs at exactly the same distance, and scipy's merge heights then tie (the condition
#: below); the seeds are the first ones for which scipy's heights meet the conditions.  "two-doors-17" draws from both sides of the cut roadmap.
SUBREGION_CASES = (("48x40@5", "48x40", 16, 1, 5.0, True), ("48x40@100", "48x40", 16, 1, 100.0, True), ("64x80@4", "64x80", 40, 24, 4.0, True),
                   ("67x130@6", "67x130", 50, 148, 6.0, True), ("two-doors-17@7", "two-doors-17", 14, 1, 7.0, False), ("single", "48x40", 1, 0, 5.0, True))


@functools.lru_cache(maxsize=None)
def subregion_case(key):
    """-> SimpleNamespace(node_rc, D (scipy's), px_per_m, t, C, labels and heights of the restatement, labels and heights of scipy)"""
    _, name, K, seed, px_per_m, reachable = next(c for c in SUBREGION_CASES if c[0] == key)
    ref = rc.reference(name)
    pixels = np.argwhere((ref.roadmap != 0) & ((ref.field_b != INF) | (not reachable))).astype(np.int32)
    node_rc = pixels[np.sort(np.random.RandomState(seed).choice(len(pixels), K, replace=False))]
    D = ref_node_distances(ref.roadmap, node_rc)
    C, thr = ref_C(node_rc, D), 2.0 * px_per_m
    labels, heights = ref_linkage(C, thr)
    sp_labels, sp_heights = scipy_labels(C, thr)
    return types.SimpleNamespace(key=key, node_rc=node_rc, D=D, px_per_m=px_per_m, t=thr, C=C, labels=labels, heights=heights, sp_labels=sp_labels,
                                 sp_heights=sp_heights)


def check_subregion_conditions():
    """what the issue asks of the case set, on scipy and the fixture alone"""
    cases = [subregion_case(c[0]) for c in SUBREGION_CASES]
    for cs in cases:
        h = np.sort(cs.sp_heights)
        assert (np.diff(h) > 1e-9 * h[1:]).all(), f"{cs.key}: two of scipy's merge heights lie within 1e-9 relative"
        assert (np.abs(h - cs.t) > 1e-9 * cs.t).all(), f"{cs.key}: a merge height lies within 1e-9 relative of t"
        assert np.array_equal(cs.D, cs.D.T)
    counts = [int(cs.sp_labels.max(initial=-1)) + 1 for cs in cases]
    assert 1 in [c for c, cs in zip(counts, cases) if len(cs.node_rc) > 1] and max(counts) >= 3, counts
    assert any((cs.D == INF).any() for cs in cases) and any(len(cs.node_rc) == 1 for cs in cases)
    gold = np.load(GOLDEN)
    for cs in cases:
        assert np.array_equal(gold[cs.key + "_node_rc"], cs.node_rc) and np.array_equal(gold[cs.key + "_D"], cs.D), "the fixture holds this case"
        assert float(gold[cs.key + "_px_per_m"]) == cs.px_per_m


def check_subregion_restatement(key):
    """the three expectations agree among themselves: the rule's restatement, scipy, the reference's recorded labels"""
    cs = subregion_case(key)
    assert np.array_equal(cs.labels, cs.sp_labels), "restatement against scipy"
    made = np.sort(cs.heights[np.isfinite(cs.heights)])
    assert np.allclose(made, np.sort(cs.sp_heights)[:len(made)], rtol=1e-12, atol=0.0)
    assert np.array_equal(canonical(np.load(GOLDEN)[key + "_labels"]), cs.labels), "restatement against the reference's get_subregions"


@guarded
def check_subregions(device, key):
    cs = subregion_case(key)
    K = len(cs.node_rc)
    labels, count, heights = RM.subregions(None, t(cs.D, device), cs.px_per_m, node_rc=t(cs.node_rc, device))
    assert labels.dtype == torch.int32 and count.dtype == torch.int32 and heights.dtype == torch.float64 and heights.shape == (K - 1,)
    got, got_h = n(labels), n(heights)
    print(f"[subregions {key}] K {K}, {int(count.item())} clusters, t {cs.t}")
    assert np.array_equal(got, cs.labels), "(a) the rule's restatement"
    assert int(count.item()) == int(cs.labels.max()) + 1
    made = np.isfinite(cs.heights)
    assert np.array_equal(np.isfinite(got_h), made) and (got_h[~made] == np.inf).all()
    assert (np.abs(got_h[made] - cs.heights[made]) <= 1e-12 * np.abs(cs.heights[made])).all(), "(a) merge heights"
    assert np.array_equal(got, cs.sp_labels), "(b) scipy's fcluster"
    assert np.array_equal(got, canonical(np.load(GOLDEN)[key + "_labels"])), "(c) the reference's get_subregions"


@guarded
def check_subregions_edges(device):
    """K = 0 and K = 2; ties (four nodes on a square, every D unreachable: equal distances) go to the smallest (a, b); a threshold of +inf"""
    labels, count, heights = RM.subregions(None, t(np.zeros((0, 0), np.int32), device), 5.0, node_rc=t(np.zeros((0, 2), np.int32), device))
    assert labels.shape == (0,) and heights.shape == (0,) and int(count.item()) == 0
    square = np.array([(0, 0), (0, 10), (10, 0), (10, 10)], np.int32)
    for D, thr in ((np.full((4, 4), INF, np.int32), 100.0), (np.full((4, 4), 120, np.int32), 6.0), (np.full((4, 4), 120, np.int32), 0.5)):
        np.fill_diagonal(D, 0)
        want, want_h = ref_linkage(ref_C(square, D), 2.0 * thr)
        labels, count, heights = RM.subregions(None, t(D, device), thr, node_rc=t(square, device))
        assert np.array_equal(n(labels), want) and int(count.item()) == int(want.max()) + 1
        assert np.array_equal(np.isfinite(n(heights)), np.isfinite(want_h)) and np.allclose(n(heights)[np.isfinite(want_h)], want_h[np.isfinite(want_h)], rtol=1e-12, atol=0)
    # more nodes than the workgroup has threads, a random symmetric D with unreachable pairs and many equal entries: the rule's restatement alone
    rng = np.random.RandomState(5)
    K = 300
    many = rng.randint(0, 200, (K, 2)).astype(np.int32)
    D = rng.randint(1, 40, (K, K)).astype(np.int32) * 12
    D[rng.rand(K, K) < 0.05] = INF
    D = np.triu(D, 1) + np.triu(D, 1).T
    want, want_h = ref_linkage(ref_C(many, D), 2.0 * 18.0)
    assert 3 <= want.max() + 1 < K
    labels, count, heights = RM.subregions(None, t(D, device), 18.0, node_rc=t(many, device))
    assert np.array_equal(n(labels), want) and int(count.item()) == int(want.max()) + 1
    made = np.isfinite(want_h)
    assert np.array_equal(np.isfinite(n(heights)), made) and (np.abs(n(heights)[made] - want_h[made]) <= 1e-12 * want_h[made]).all()
    two = np.array([(3, 3), (3, 9)], np.int32)
    D2 = np.array([[0, 72], [72, 0]], np.int32)
    labels, count, heights = RM.subregions(None, t(D2, device), math.inf, node_rc=t(two, device))
    assert n(labels).tolist() == [0, 0] and int(count.item()) == 1 and n(heights).tolist() == [6.0]
    labels, count, heights = RM.subregions(None, t(D2, device), 1.0, node_rc=t(two, device))
    assert n(labels).tolist() == [0, 1] and int(count.item()) == 2 and n(heights).tolist() == [math.inf]


@guarded
def check_repeatable(device):
    """two runs give the same bytes, output by output"""
    cs = subregion_case("67x130@6")
    ref = rc.reference("67x130")
    runs = []
    for _ in range(2):
        D = RM.node_distances(t(ref.roadmap, device), t(cs.node_rc, device))
        labels, count, heights = RM.subregions(None, D, cs.px_per_m, node_rc=t(cs.node_rc, device))
        clear = RM.segment_clearance(t(ref.dist2, device), t(segment_set(*ref.dist2.shape), device))
        runs.append([n(x).tobytes() for x in (D, labels, count, heights, clear)])
    assert runs[0] == runs[1]


@guarded
def check_refusals(device):
    """K above the limit, wrong dtypes and shapes raise in Python; the C entry points refuse what they name before any launch"""
    ref = rc.reference("48x40")
    H, W = ref.roadmap.shape
    mask, dist2 = t(ref.roadmap, device), t(ref.dist2, device)
    many = torch.zeros(RM.MAX_NODES + 1, 2, dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="at most 1024"):
        RM.node_distances(mask, many)
    with pytest.raises(ValueError, match="at most 1024"):
        RM.subregions(None, torch.zeros(1, 1, dtype=torch.int32, device=device), 5.0, node_rc=many)
    with pytest.raises(ValueError, match="int32"):
        RM.node_distances(mask, many[:3].to(torch.int64))
    with pytest.raises(ValueError, match="segments"):
        RM.segment_clearance(dist2, torch.zeros(3, 2, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="int32"):
        RM.segment_clearance(mask, torch.zeros(3, 4, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match=r"\[3, 3\]"):
        RM.subregions(None, torch.zeros(3, 2, dtype=torch.int32, device=device), 5.0, node_rc=many[:3].contiguous())
    with pytest.raises(ValueError, match="not negative"):
        RM.subregions(None, torch.zeros(3, 3, dtype=torch.int32, device=device), 5.0, path_weight=-1.0, node_rc=many[:3].contiguous())
    lib, st, p = _lib.get(), _lib.stream_ptr(torch.device(device)), R._ptr
    scratch = torch.zeros(int(lib.gs_node_distances_scratch_bytes(H, W)), dtype=torch.uint8, device=device)
    out = torch.zeros(16, dtype=torch.int32, device=device)
    dbl = torch.zeros(16, dtype=torch.float64, device=device)
    assert lib.gs_node_distances_scratch_bytes(0, 5) == 0 and lib.gs_node_distances_scratch_bytes(4096, 4096) >= 16 * 4096 * 4096
    assert lib.gs_subregions_scratch_bytes(1025) == 0 and lib.gs_subregions_scratch_bytes(1024) >= 8 * 1024 * 1024
    assert lib.gs_node_distances(H, W, p(mask), 1025, p(many), p(out), p(scratch), st) == GS_EINVAL
    assert "node count out of range" in lib.gs_last_error().decode()
    assert lib.gs_node_distances(H, W, p(mask), -1, p(many), p(out), p(scratch), st) == GS_EINVAL
    assert lib.gs_node_distances(0, W, p(mask), 2, p(many), p(out), p(scratch), st) == GS_EINVAL
    assert lib.gs_node_distances(H, W, None, 2, p(many), p(out), p(scratch), st) == GS_EINVAL
    assert lib.gs_node_distances(H, W, p(mask), 2, None, p(out), p(scratch), st) == GS_EINVAL
    assert lib.gs_node_distances(H, W, p(mask), 2, p(many), p(out), None, st) == GS_EINVAL
    assert lib.gs_node_distances(H, W, p(mask), 2, p(many), p(out), scratch.data_ptr() + 4, st) == GS_EINVAL
    assert lib.gs_node_distances(H, W, p(mask), 2, p(many), out.data_ptr() + 2, p(scratch), st) == GS_EINVAL
    assert lib.gs_segment_clearance(H, 4097, p(dist2), 1, p(out), p(out), st) == GS_EINVAL
    assert lib.gs_segment_clearance(H, W, p(dist2), -1, p(out), p(out), st) == GS_EINVAL
    assert lib.gs_segment_clearance(H, W, None, 1, p(out), p(out), st) == GS_EINVAL
    assert lib.gs_segment_clearance(H, W, p(dist2), 1, None, p(out), st) == GS_EINVAL
    assert lib.gs_segment_clearance(H, W, p(dist2), 1, p(out), out.data_ptr() + 1, st) == GS_EINVAL
    ok = dict(K=2, node_rc=p(many), D=p(out), pw=0.5, cw=0.5, t=10.0, labels=p(out), count=p(out), heights=p(dbl), scratch=p(scratch))
    for bad in (dict(K=1025), dict(K=-1), dict(pw=-0.5), dict(cw=math.inf), dict(t=math.nan), dict(t=-1.0), dict(node_rc=None), dict(D=None),
                dict(labels=None), dict(count=None), dict(heights=None), dict(scratch=None), dict(heights=dbl.data_ptr() + 4)):
        a = dict(ok); a.update(bad)
        assert lib.gs_subregions(a["K"], a["node_rc"], a["D"], a["pw"], a["cw"], a["t"], a["labels"], a["count"], a["heights"], a["scratch"], st) == GS_EINVAL, bad
    assert "gs_subregions" in lib.gs_last_error().decode()
    assert not n(out).any() and not n(dbl).any() and not n(scratch).any(), "nothing was launched"


# ---- policy (host) ---------------------------------------------------------------------------------------------------------------------------------

def ref_scores(inv, vol, unarrived, in_horizon, fail):
    """planner_node.py:1201-1215 with the initial weights, element by element; a zero or NaN maximum gives a term of 0"""
    def scaled(v):
        finite = [x for x in v if not math.isnan(x)]
        top = max(finite) if finite else math.nan
        if not finite or top == 0 or not math.isfinite(top):
            return [0] * len(v)
        return [0 if math.isnan(x) else math.ceil(x / top * 10) for x in v]
    si, sv = scaled(list(inv)), scaled(list(vol))
    score = [20 * int(u) + 10 * int(h) + 2 * a + 1 * b - 60 * int(f) for u, h, a, b, f in zip(unarrived, in_horizon, si, sv, fail)]
    return np.array(score, np.int32), np.array([0 if math.isnan(x) else math.ceil(x) for x in inv], np.int32)


def check_node_scores():
    rng = np.random.RandomState(3)
    K = 17
    inv, vol = rng.rand(K) * 400.0, rng.rand(K) * 3.0
    flags = [rng.randint(0, 2, K) for _ in range(3)]
    for i, v in ((inv, vol), (inv, np.zeros(K)), (np.zeros(K), vol), (np.where(np.arange(K) == 2, np.nan, inv), vol), (inv[:0], vol[:0])):
        f = [x[:len(i)] for x in flags]
        score, inv_score = PL.node_scores(i, v, *f)
        want, want_inv = ref_scores(i, v, *f)
        assert score.dtype == np.int32 and inv_score.dtype == np.int32 and np.array_equal(score, want) and np.array_equal(inv_score, want_inv)
    score, _ = PL.node_scores(inv, np.zeros(K), np.ones(K), np.zeros(K), np.zeros(K))
    assert score.max() == 20 + 2 * 10 and score.min() >= 20, "an all-zero volume adds nothing"
    pol = PL.SubregionPolicy(step_px=2.0, radius_px=3.0, visited_steps=10)
    assert (pol.arrived_px, pol.visited_px, pol.too_far_px) == (3.0, 20.0, 400.0)
    nodes = np.array([(0, 0), (0, 25), (30, 0)])
    assert pol.flags(nodes)[0].tolist() == [1, 1, 1] and pol.flags(nodes)[1].tolist() == [0, 0, 0]
    pol.visit((0, 4)); pol.fail((30, 3)); pol.fail((0, 21))
    assert pol.flags(nodes)[0].tolist() == [0, 1, 1] and pol.flags(nodes)[1].tolist() == [0, 0, 1]


def scenario():
    """six nodes in three subregions along a line (labels 0 0 1 1 2 2), the agent beside node 0; D = 12 x the distance along the line"""
    node_rc = np.array([(10, 10), (10, 20), (10, 60), (10, 70), (10, 120), (10, 130)], np.int32)
    D = (12 * np.abs(node_rc[:, None, 1] - node_rc[None, :, 1])).astype(np.int32)
    rm = types.SimpleNamespace(agent_rc=(10, 8), node_rc=node_rc)
    labels = np.array([0, 0, 1, 1, 2, 2], np.int32)
    length = (node_rc[:, 1] - 8).astype(np.float64)
    return rm, D, labels, length


def check_choose():
    """one scenario per branch of SubregionPolicy.choose"""
    rm, D, labels, length = scenario()
    new = lambda **k: PL.SubregionPolicy(step_px=1.0, radius_px=2.0, arrived_steps=1.5, **k)       # arrived within 1.5 px, too far beyond 200 px
    high = np.array([300, 300, 300, 300, 300, 300])
    # local plan: the current subregion still holds an invisibility score >= 250; the best score of subregion 0 wins although 4 scores more
    pol = new()
    assert pol.choose(rm, (D, labels), [30, 32, 10, 10, 50, 10], high, length) == 1 and pol.last["plan"] == "local" and pol.last["current"] == 0
    # global plan because the maximum is below 250: the subregion with the best score, then its best node
    pol = new()
    assert pol.choose(rm, (D, labels), [30, 32, 10, 12, 50, 10], [249, 100, 300, 300, 300, 300], length) == 4
    assert pol.last["plan"] == "global" and pol.last["subregion"] == 2
    # ... a score <= 0 takes the invisibility score away: 300 at node 1 does not keep the plan local
    pol = new()
    assert pol.choose(rm, (D, labels), [30, 0, 10, 12, 5, 10], [100, 300, 300, 300, 300, 300], length) == 3 and pol.last["plan"] == "global"
    # global plan because everything in the current subregion is arrived (selected positions on both nodes), whatever the scores
    pol = new()
    pol.arrive((10, 10)); pol.arrive((10, 20))
    assert pol.choose(rm, (D, labels), [30, 32, 10, 12, 5, 11], high, length) == 3 and pol.last["plan"] == "global" and pol.last["subregion"] == 1
    # ... and an arrived node outside the current subregion does not count for its subregion: 2's best is then 10, 1's 12
    pol = new()
    pol.arrive((10, 10)); pol.arrive((10, 20)); pol.arrive((10, 120))
    assert pol.choose(rm, (D, labels), [30, 32, 10, 12, 50, 10], high, length) == 3
    # the first subregion wins a tie of the maxima
    pol = new()
    assert pol.choose(rm, (D, labels), [1, 1, 7, 3, 7, 7], [0] * 6, length) == 2 and pol.last["subregion"] == 1
    # use_global_plan forces the global plan once
    pol = new()
    pol.use_global_plan = True
    assert pol.choose(rm, (D, labels), [30, 32, 10, 12, 50, 10], high, length) == 4 and pol.use_global_plan is False
    # a tie of the scores is broken by the shorter path; a node the agent stands on is skipped
    pol = new()
    assert pol.choose(rm, (D, labels), [32, 32, 10, 10, 50, 10], high, length) == 0
    near = types.SimpleNamespace(agent_rc=(10, 10), node_rc=rm.node_rc)
    assert new().choose(near, (D, labels), [32, 32, 10, 10, 50, 10], high, length) == 1
    # too far, remembered, then taken at a lower level: node 5 (score 50) lies 300 px away; node 4 (score 40) within the bound and nearer
    # to node 5 than node 5 is to the agent
    far_len = np.array([2.0, 12.0, 52.0, 62.0, 112.0, 300.0])
    pol = new()
    pol.use_global_plan = True
    assert pol.choose(rm, (D, labels), [1, 1, 2, 2, 40, 50], [0] * 6, far_len) == 4 and pol.last["far"] == 5
    # too far and returned at the end: nothing at a lower level lies within the bound
    pol = new()
    pol.use_global_plan = True
    assert pol.choose(rm, (D, labels), [1, 1, 2, 2, 40, 50], [0] * 6, np.array([2.0, 12.0, 52.0, 62.0, 250.0, 300.0])) == 5
    # ... or lies within the bound but no nearer to the far target than the target's own path (D unreachable)
    cut = D.copy()
    cut[4, 5] = cut[5, 4] = INF
    pol = new()
    pol.use_global_plan = True
    assert pol.choose(rm, (cut, labels), [1, 1, 2, 2, 40, 50], [0] * 6, far_len) == 5
    # nothing reachable -> -1, and the next call plans globally
    pol = new()
    assert pol.choose(rm, (D, labels), [30, 32, 10, 12, 50, 10], high, np.full(6, np.nan)) == -1 and pol.use_global_plan is True
    empty = types.SimpleNamespace(agent_rc=(10, 8), node_rc=np.zeros((0, 2), np.int32))
    assert new().choose(empty, (np.zeros((0, 0), np.int32), np.zeros(0, np.int32)), [], [], []) == -1


# ---- GPU only: through the rasteriser ---------------------------------------------------------------------------------------------------------------

@guarded
def check_mapper_plan_step_policy(device):
    """the scene of roadmap_cases.check_mapper_plan_step: policy=None is the call without the argument, byte for byte; with a policy the
    node is a member of the chosen subregion, the shortcut is safe, the waypoints start at the agent, and two runs give the same bytes"""
    params, wall = rc.splat_room(device)
    mp = rc.mapper_of(params, device)
    agent_rc = (24, 10)
    ax, az = RM.pixel_to_world(np.array(agent_rc), **rc.WORLD)
    c2w = np.eye(4)
    c2w[:3, 3] = [ax, -0.5, az]
    view = torch.tensor(c2w, dtype=torch.float32)
    kw = dict(upper=rc.BAND[0], lower=rc.BAND[1], agent_radius=0.25, node_spacing=1.0, scale_modifier=1.0, **rc.WORLD)
    plain, none = mp.plan_step(view, **kw), mp.plan_step(view, policy=None, **kw)
    assert set(plain) == set(none) == {"roadmap", "positions", "invisibility", "volume", "node", "path_rc", "waypoints"} and plain["node"] == none["node"]
    for key in ("positions", "invisibility", "volume"):
        assert plain[key].tobytes() == none[key].tobytes(), key
    for key in ("path_rc", "waypoints"):
        assert plain[key].dtype == none[key].dtype and n(plain[key]).tobytes() == n(none[key]).tobytes(), key
    runs = []
    for _ in range(2):
        pol = PL.SubregionPolicy(step_px=2.0, radius_px=0.25 * 8.0)
        step = mp.plan_step(view, policy=pol, **kw)
        rm, node = step["roadmap"], step["node"]
        assert rm.K >= 4 and 0 <= node < rm.K and np.array_equal(n(rm.node_rc), n(plain["roadmap"].node_rc))
        labels = step["subregions"]
        assert labels.shape == (rm.K,) and labels[node] == pol.last["subregion"] and node in pol.last["candidates"]
        want_D = ref_node_distances(n(rm.roadmap), n(rm.node_rc))
        assert np.array_equal(n(step["distances"]), want_D)
        assert np.array_equal(labels, ref_linkage(ref_C(n(rm.node_rc), want_D), 2.0 * rm.px_per_m)[0])
        assert step["scores"].shape == (rm.K,) and step["scores"].dtype == np.int32
        assert int(step["safe"].item()) == 1
        short, way = n(step["shortcut_rc"]), n(step["waypoints"])
        assert tuple(short[0]) == agent_rc and tuple(short[-1]) == tuple(n(rm.node_rc)[node]) and way.shape == (len(short), 3)
        assert np.array_equal(np.rint(RM.world_to_pixel(way[:, [0, 2]].astype(np.float64), **rc.WORLD)).astype(np.int32), short) and (way[:, 1] == -0.5).all()
        path = n(step["path_rc"])
        assert tuple(path[0]) == agent_rc and np.array_equal(path[len(path) - (len(short) - 1):], short[1:])
        assert len(pol.visited) == 1 and tuple(pol.visited[0]) == agent_rc
        runs.append([node, labels.tobytes(), step["scores"].tobytes()] + [n(step[k]).tobytes() for k in ("distances", "path_rc", "shortcut_rc", "safe", "waypoints")])
    assert runs[0] == runs[1]


def check_no_cpu_fallback():
    _lib.unload_for_tests()
    ref = rc.reference("48x40")
    mask, dist2, nodes = torch.from_numpy(ref.roadmap), torch.from_numpy(ref.dist2), torch.from_numpy(ref.node_rc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.node_distances(mask, nodes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.segment_clearance(dist2, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.subregions(None, torch.zeros(len(nodes), len(nodes), dtype=torch.int32), 5.0, node_rc=nodes)
    rm = types.SimpleNamespace(agent_rc=(5, 5), node_rc=nodes, dist2=dist2, trav=mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.nodes_in_horizon(rm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RM.shortcut_path(rm, nodes, 2.0)
