"""Shared checks of the planner roadmap (activesplat_amd/roadmap.py; gs_traversable_map, gs_clearance_field, gs_voronoi_roadmap, gs_grid_geodesic,
gs_roadmap_entry, gs_roadmap_nodes, gs_trace_path): run on the host-emulated kernels by tests/test_roadmap.py and on the MI355X by
tests/test_gpu_roadmap.py, every check inside guard.guarded_allocations.

The stage is a grid formulation written for this package, not a restatement of the reference's host chain: nothing here is pinned to the
reference.  Everything is integers and EVERY comparison is exact equality.  Expected values come from scipy where scipy has the operation and
from numpy restatements of the rules of include/gsplat_hip.h elsewhere; nothing from the code under test goes into them:

* traversable map   scipy.ndimage.binary_opening (open_size x open_size structure: equal to the union of the squares inside the mask),
                    binary_dilation, label with 8-connectivity;
* dist2             scipy.ndimage.distance_transform_edt of the map padded by one zero ring, squared and rounded;
* feature           brute force over the obstacles in lexicographic order (np.argmin takes the first minimum);
* geodesic fields   scipy.sparse.csgraph.dijkstra on the same integer weights (exact in float64: lengths stay far below 2^53);
* roadmap, entry, nodes, paths   numpy restatements (`ref_roadmap`, `ref_entry`, `ref_nodes`, `ref_trace`).
A case's references are computed once (`reference`) and shared by the checks; they are not modified.
"""
import functools
import types

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

from activesplat_amd import _lib
from activesplat_amd import rasterizer as R
from activesplat_amd import roadmap as RM
from tests import guard

GS_EINVAL = 1
INF = RM.UNREACHABLE
STEPS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))          # the order gs_trace_path tries


def guarded(check):
    """the check inside guard.guarded_allocations: bands around every device allocation"""
    def run(device, *a, **k):
        with guard.guarded_allocations(torch.device(device), poison="float_nan"):
            return check(device, *a, **k)
    run.__name__ = check.__name__
    run.__doc__ = check.__doc__
    return run


def t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).contiguous()


def n(x):
    return x.detach().cpu().numpy()


# ---- maps --------------------------------------------------------------------------------------------------------------------------------------

def floor_plan(H, W, seed):
    """A seeded floor plan: a 3-pixel border, wall strips (4 to 5 pixels thick: the 3 x 3 dilation erases a 2-pixel wall from both sides) with
    doors, boxes, 1 % speckle; the left columns are unseen.  -> (free, unseen) uint8"""
    rng = np.random.RandomState(seed)
    free = np.zeros((H, W), np.uint8)
    free[3:H - 3, 3:W - 3] = 1
    for k in range(max(1, W // 28)):                                   # vertical walls with two doors each
        c = int(rng.randint(12, W - 16)); th = int(rng.randint(4, 6))
        free[:, c:c + th] = 0
        for _ in range(2):
            r = int(rng.randint(4, H - 12)); free[r:r + int(rng.randint(4, 8)), c:c + th] = 1
    for k in range(max(1, H // 30)):                                   # horizontal walls with two doors each
        r = int(rng.randint(12, H - 16)); th = int(rng.randint(4, 6))
        free[r:r + th, :] = 0
        for _ in range(2):
            c = int(rng.randint(4, W - 12)); free[r:r + th, c:c + int(rng.randint(4, 8))] = 1
    for k in range(3):                                                 # boxes
        r, c = int(rng.randint(4, H - 10)), int(rng.randint(4, W - 10))
        free[r:r + int(rng.randint(4, 7)), c:c + int(rng.randint(4, 7))] = 0
    free[rng.rand(H, W) < 0.01] = 0
    free[:3] = 0; free[H - 3:] = 0; free[:, :3] = 0; free[:, W - 3:] = 0
    unseen = np.zeros((H, W), np.uint8)
    unseen[:, :5] = 1
    return free, unseen


def roomiest_pixel(free, unseen):
    """the pixel of free-and-seen space farthest from its complement (the first in row-major order): where the cases put the agent"""
    d = ndimage.distance_transform_edt(np.pad((free != 0) & (unseen == 0), 1))[1:-1, 1:-1]
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(d)), d.shape))


def two_doors():
    free = np.zeros((48, 40), np.uint8)
    free[3:45, 3:37] = 1
    free[:, 18:22] = 0
    free[10:14, 18:22] = 1
    free[30:36, 18:22] = 1
    unseen = np.zeros((48, 40), np.uint8)
    unseen[40:, 30:] = 1
    return free, unseen


def serpentine(S=96, lane=6, wall=4):
    """corridors of `lane` pixels between walls of `wall` pixels that run the whole width but for a gap at alternating ends: the way from the
    first corridor to the last crosses the 32-pixel relaxation tiles many times"""
    mask = np.zeros((S, S), np.uint8)
    mask[2:S - 2, 2:S - 2] = 1
    r, k = 2 + lane, 0
    while r + wall + lane <= S - 2:
        mask[r:r + wall, :] = 0
        if k % 2 == 0:
            mask[r:r + wall, S - 2 - lane:S - 2] = 1
        else:
            mask[r:r + wall, 2:2 + lane] = 1
        r += wall + lane; k += 1
    return mask


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(free, unseen, agent, open_size, dilate, min_dist2, cell)"""
    mk = lambda free, unseen, agent, open_size=4, dilate=3, min_dist2=4, cell=8: types.SimpleNamespace(
        name=name, free=free, unseen=unseen, agent=agent, open_size=open_size, dilate=dilate, min_dist2=min_dist2, cell=cell)
    if name in ("48x40", "64x80", "67x130"):
        H, W = (int(v) for v in name.split("x"))
        free, unseen = floor_plan(H, W, seed=H)
        return mk(free, unseen, roomiest_pixel(free, unseen))
    if name == "1x1":
        return mk(np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8), (0, 0), 1, 1, 0, 1)
    if name in ("1x70", "70x1"):                                       # a line with one obstacle pixel; no 4 x 4 square fits: open_size 1
        free = np.ones(70, np.uint8); free[40] = 0
        shape = (1, 70) if name == "1x70" else (70, 1)
        return mk(free.reshape(shape), np.zeros(shape, np.uint8), (0, 5) if name == "1x70" else (5, 0), 1, 1, 1, 8)
    if name == "all-obstacle":
        return mk(np.zeros((48, 40), np.uint8), np.zeros((48, 40), np.uint8), (24, 20))
    if name == "all-free":
        return mk(np.ones((64, 80), np.uint8), np.zeros((64, 80), np.uint8), (30, 41))
    if name.startswith("two-doors-"):
        free, unseen = two_doors()
        return mk(free, unseen, (24, 8), min_dist2=int(name.split("-")[-1]))
    raise KeyError(name)


CASES = ("48x40", "64x80", "67x130", "1x1", "1x70", "70x1", "all-obstacle", "all-free")


# ---- the rules, restated -------------------------------------------------------------------------------------------------------------------------

def ref_traversable(free, unseen, agent, open_size, dilate):
    m0 = (free != 0) & (unseen == 0)
    opened = ndimage.binary_opening(m0, structure=np.ones((open_size, open_size), bool))
    dil = ndimage.binary_dilation(opened, structure=np.ones((dilate, dilate), bool))
    labels, _ = ndimage.label(dil, structure=np.ones((3, 3), bool))
    if not dil[agent]:
        return np.zeros(free.shape, np.uint8), 1
    return (labels == labels[agent]).astype(np.uint8), 0


def brute_opening(m0, s):
    """the union of all s x s squares that lie wholly inside the image and inside m0, by its definition"""
    H, W = m0.shape
    out = np.zeros((H, W), bool)
    for r in range(H - s + 1):
        for c in range(W - s + 1):
            if m0[r:r + s, c:c + s].all():
                out[r:r + s, c:c + s] = True
    return out


def ref_clearance(trav):
    """-> (dist2 int32 from scipy's EDT, feature int16 by brute force, dist2 by brute force, pixels with two or more equidistant obstacles)"""
    H, W = trav.shape
    padded = np.pad(trav != 0, 1)
    edt = ndimage.distance_transform_edt(padded)[1:-1, 1:-1]
    dist2 = np.rint(edt * edt).astype(np.int32)
    obs = np.argwhere(~padded).astype(np.int64) - 1                    # lexicographic (r, c) order; the frame is rows / columns -1, H, W
    feature = np.zeros((H, W, 2), np.int16)
    brute = np.zeros((H, W), np.int32)
    ties = 0
    cols = np.arange(W, dtype=np.int64)
    for r in range(H):
        d = (r - obs[:, 0])[None, :] ** 2 + (cols[:, None] - obs[None, :, 1]) ** 2          # [W, obstacles]
        k = np.argmin(d, axis=1)                                                              # the first minimum: the smallest (r, c)
        best = d[cols, k]
        feature[r] = obs[k]
        brute[r] = best
        ties += int(((d == best[:, None]).sum(1) >= 2).sum())
    return dist2, feature, brute, ties


def ref_roadmap(trav, dist2, feature, min_dist2, gamma2=4):
    H, W = trav.shape
    f = feature.astype(np.int64)
    rc = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), -1).astype(np.int64)
    marked = np.zeros((H, W), bool)
    for axis in (0, 1):
        sl_p = (slice(0, H - 1), slice(None)) if axis == 0 else (slice(None), slice(0, W - 1))
        sl_q = (slice(1, H), slice(None)) if axis == 0 else (slice(None), slice(1, W))
        p, q, fp, fq = rc[sl_p], rc[sl_q], f[sl_p], f[sl_q]
        pair = (trav[sl_p] != 0) & (trav[sl_q] != 0) & (((fp - fq) ** 2).sum(-1) > gamma2)
        ap, aq = ((p + q - 2 * fp) ** 2).sum(-1), ((p + q - 2 * fq) ** 2).sum(-1)
        marked[sl_p] |= pair & (aq <= ap)
        marked[sl_q] |= pair & (ap <= aq)
    return (marked & (dist2 >= min_dist2)).astype(np.uint8)


def ref_geodesic(mask, seed):
    """scipy's Dijkstra over the 8-connected pixels of the mask, straight 12, diagonal 17 -> (int32 field, status bit)"""
    H, W = mask.shape
    field = np.full((H, W), INF, np.int32)
    m = mask != 0
    if not (0 <= seed[0] < H and 0 <= seed[1] < W) or not m[seed]:
        return field, 2
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, w = [], [], []
    for dr, dc in STEPS:
        a = (slice(max(0, -dr), H - max(0, dr)), slice(max(0, -dc), W - max(0, dc)))
        b = (slice(max(0, dr), H - max(0, -dr)), slice(max(0, dc), W - max(0, -dc)))
        ok = m[a] & m[b]
        rows.append(idx[a][ok]); cols.append(idx[b][ok]); w.append(np.full(int(ok.sum()), 17.0 if dr and dc else 12.0))
    g = coo_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W)).tocsr()
    d = dijkstra(g, directed=True, indices=seed[0] * W + seed[1])
    field.reshape(-1)[np.isfinite(d)] = d[np.isfinite(d)].astype(np.int32)
    return field, 0


def ref_entry(roadmap, field):
    """(r, c, field) of the roadmap pixel with the smallest finite field, the smallest index on a tie; (-1, -1, INF) without one"""
    ok = (roadmap != 0) & (field != INF)
    if not ok.any():
        return -1, -1, INF
    key = np.where(ok, field.astype(np.int64), np.int64(INF)).reshape(-1)
    p = int(np.argmin(key))
    return p // roadmap.shape[1], p % roadmap.shape[1], int(key[p])


def ref_nodes(roadmap, dist2, field, cell):
    H, W = roadmap.shape
    rc, d2, fv = [], [], []
    for r0 in range(0, H, cell):
        for c0 in range(0, W, cell):
            ok = (roadmap[r0:r0 + cell, c0:c0 + cell] != 0) & (field[r0:r0 + cell, c0:c0 + cell] != INF)
            if not ok.any():
                continue
            d = np.where(ok, dist2[r0:r0 + cell, c0:c0 + cell].astype(np.int64), -1)
            k = int(np.argmax(d))                                      # the first maximum in the block's row-major order = the smallest index
            r, c = r0 + k // d.shape[1], c0 + k % d.shape[1]
            rc.append((r, c)); d2.append(int(dist2[r, c])); fv.append(int(field[r, c]))
    return np.array(rc, np.int32).reshape(-1, 2), np.array(d2, np.int32), np.array(fv, np.int32)


def ref_trace(mask, field, target):
    H, W = mask.shape
    r, c = target
    if not (0 <= r < H and 0 <= c < W) or not mask[r, c] or field[r, c] == INF:
        return np.zeros((0, 2), np.int32), 1
    out = [(r, c)]
    while field[r, c] != 0:
        for dr, dc in STEPS:
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and mask[rr, cc] and field[rr, cc] != INF and int(field[rr, cc]) + (17 if dr and dc else 12) == int(field[r, c]):
                r, c = rr, cc
                break
        else:
            raise AssertionError("the reference field is not a field of this mask")
        out.append((r, c))
    return np.array(out, np.int32), 0


def path_weight(path, mask):
    """consecutive pixels adjacent and in the mask -> (sum of the step weights, straight steps, diagonal steps)"""
    assert all(mask[r, c] for r, c in path)
    d = np.abs(np.diff(path.astype(np.int64), axis=0))
    assert d.max(initial=0) <= 1 and (d.sum(1) >= 1).all()
    diag = int((d.sum(1) == 2).sum())
    return 12 * (len(d) - diag) + 17 * diag, len(d) - diag, diag


@functools.lru_cache(maxsize=None)
def reference(name):
    """the whole chain of one case on the host, computed once"""
    cs = case(name)
    trav, st0 = ref_traversable(cs.free, cs.unseen, cs.agent, cs.open_size, cs.dilate)
    dist2, feature, brute, ties = ref_clearance(trav)
    assert np.array_equal(dist2, brute), "scipy's EDT of the padded map against brute force"
    roadmap = ref_roadmap(trav, dist2, feature, cs.min_dist2)
    field_a, st1 = ref_geodesic(trav, cs.agent)
    er, ec, ef = ref_entry(roadmap, field_a)
    field_b, st2 = ref_geodesic(roadmap, (er, ec))
    node_rc, node_d2, node_f = ref_nodes(roadmap, dist2, field_b, cs.cell)
    status = st0 | st1 | (RM.STATUS_NO_ENTRY if st2 else 0)
    return types.SimpleNamespace(trav=trav, dist2=dist2, feature=feature, ties=ties, roadmap=roadmap, field_a=field_a, entry=(er, ec), entry_field=ef,
                                 field_b=field_b, node_rc=node_rc, node_dist2=node_d2, node_field=node_f, status=status)


def check_reference_conditions():
    """what the issue asks of the case set, on the references alone"""
    rng = np.random.RandomState(0)
    m0 = rng.rand(23, 31) < 0.8
    assert np.array_equal(ndimage.binary_opening(m0, structure=np.ones((4, 4), bool)), brute_opening(m0, 4))
    for name in ("48x40", "64x80", "67x130"):
        ref = reference(name)
        assert ref.ties > 0, "pixels with two or more equidistant obstacles"
        assert 0 < ref.trav.sum() < ref.trav.size and ref.roadmap.sum() > 0 and len(ref.node_rc) >= 3 and ref.status == 0
        straight = diag = 0
        for k in range(len(ref.node_rc)):
            pb, _ = ref_trace(ref.roadmap, ref.field_b, tuple(ref.node_rc[k]))
            _, s, d = path_weight(pb, ref.roadmap)
            straight += s; diag += d
        assert straight > 0 and diag > 0, "the path cases hold both step kinds"
    assert reference("all-obstacle").status == (RM.STATUS_AGENT_OFF_MAP | RM.STATUS_SEED_OFF_MASK | RM.STATUS_NO_ENTRY)
    assert reference("all-free").trav.all() and reference("1x70").trav.sum() == 40 and reference("70x1").trav.sum() == 40


# ---- the checks --------------------------------------------------------------------------------------------------------------------------------

def run_stages(device, name):
    """the public stage functions one after the other on the case's maps -> SimpleNamespace of numpy results"""
    cs = case(name)
    status = torch.zeros(4, dtype=torch.int32, device=device)
    trav = RM.traversable_map(t(cs.free, device), t(cs.unseen, device), cs.agent, cs.open_size, cs.dilate, status=status[0:1])
    dist2, feature = RM.clearance_field(trav)
    roadmap = RM.voronoi_roadmap(trav, dist2, feature, cs.min_dist2)
    field_a, rounds_a = RM.grid_geodesic(trav, cs.agent, status=status[1:2], return_rounds=True)
    return types.SimpleNamespace(trav=trav, dist2=dist2, feature=feature, roadmap=roadmap, field_a=field_a, rounds_a=rounds_a, status=status)


def case_checked(device, name):
    """every stage of one case against its reference, stage by stage and through plan_roadmap; every node's path -> the Roadmap"""
    cs, ref = case(name), reference(name)
    H, W = cs.free.shape
    got = run_stages(device, name)
    assert np.array_equal(n(got.trav), ref.trav), "traversable map"
    assert got.dist2.dtype == torch.int32 and np.array_equal(n(got.dist2), ref.dist2), "dist2"
    assert got.feature.dtype == torch.int16 and np.array_equal(n(got.feature), ref.feature), "feature"
    assert np.array_equal(n(got.roadmap), ref.roadmap), "roadmap"
    assert np.array_equal(n(got.field_a), ref.field_a), "field A"
    assert 0 <= got.rounds_a < max(1, int(ref.trav.sum()))
    maps = types.SimpleNamespace(free_map_binary=t(cs.free, device), visible_map_binary=t(cs.unseen, device))
    radius_px = float(np.sqrt(max(0.0, cs.min_dist2 - 0.5)))           # ceil(radius_px^2) is min_dist2 whatever the square root's rounding
    rm = RM.plan_roadmap(maps, cs.agent, radius_px, cs.cell, cs.open_size, cs.dilate)
    assert rm.min_dist2 == cs.min_dist2
    for key in ("trav", "dist2", "feature", "roadmap"):
        assert np.array_equal(n(getattr(rm, key)), getattr(ref, key)), key
    assert np.array_equal(n(rm.field_agent), ref.field_a) and np.array_equal(n(rm.field_entry), ref.field_b), "fields"
    assert rm.entry_rc == ref.entry and rm.entry_field == ref.entry_field and rm.status == ref.status
    assert rm.K == len(ref.node_rc) and rm.node_rc.dtype == torch.int32
    assert np.array_equal(n(rm.node_rc), ref.node_rc) and np.array_equal(n(rm.node_dist2), ref.node_dist2) and np.array_equal(n(rm.node_field), ref.node_field)
    # the stage functions alone, on the reference's arrays
    node_rc, node_d2, node_f, count = RM.roadmap_nodes(t(ref.roadmap, device), t(ref.dist2, device), t(ref.field_b, device), cs.cell)
    K = int(count.item())
    assert K == len(ref.node_rc) and np.array_equal(n(node_rc[:K]), ref.node_rc) and np.array_equal(n(node_d2[:K]), ref.node_dist2)
    pa_ref, st = ref_trace(ref.trav, ref.field_a, ref.entry)
    pa, sa = RM.trace_path(rm.trav, rm.field_agent, ref.entry, H * W, return_status=True)
    assert sa == st and np.array_equal(n(pa), pa_ref)
    lengths = n(rm.node_path_length()) if rm.K else np.zeros(0, np.int64)
    for k in range(rm.K):
        pb_ref, st = ref_trace(ref.roadmap, ref.field_b, tuple(ref.node_rc[k]))
        assert st == 0
        pb, sb = RM.trace_path(rm.roadmap, rm.field_entry, tuple(int(v) for v in ref.node_rc[k]), H * W, return_status=True)
        assert sb == 0 and np.array_equal(n(pb), pb_ref)
        assert path_weight(n(pb), ref.roadmap)[0] == ref.node_field[k]
        want = np.concatenate([pb_ref, pa_ref[1:]])[::-1]
        path = n(rm.path_to(k))
        assert np.array_equal(path, want)
        assert tuple(path[0]) == tuple(cs.agent) and tuple(path[-1]) == tuple(ref.node_rc[k])
        assert path_weight(path, ref.trav)[0] == int(ref.entry_field) + int(ref.node_field[k]) == int(lengths[k])
    # a trace that runs out of capacity, and one from an unreachable target
    if rm.K and len(pa_ref) > 1:
        short, s2 = RM.trace_path(rm.trav, rm.field_agent, ref.entry, len(pa_ref) - 1, return_status=True)
        assert s2 == 2 and np.array_equal(n(short), pa_ref[:-1])
    off = np.argwhere(ref.trav == 0)
    if len(off):
        none, s1 = RM.trace_path(rm.trav, rm.field_agent, tuple(int(v) for v in off[0]), 16, return_status=True)
        assert s1 == 1 and len(none) == 0
    return rm


check_case = guarded(case_checked)


def two_doors_figures(ref):
    """(cells that hold a roadmap pixel, nodes = those a path from the entry reaches, the largest finite field B)"""
    everywhere = np.zeros(ref.field_b.shape, np.int32)
    finite = ref.field_b[ref.field_b != INF]
    return len(ref_nodes(ref.roadmap, ref.dist2, everywhere, 8)[0]), len(ref.node_rc), int(finite.max())


@guarded
def check_two_doors(device):
    """48 x 40, a wall with a narrow (4 pixel) and a wide (6 pixel) door: at min_dist2 9 the roadmap runs through both doors; at 10 the narrow
    door's roadmap is cut and the way round grows; at 17 the wide door is cut too and only the agent's side is reachable.  "Reachable" counts
    the cells that hold a roadmap pixel (roadmap_nodes with an all-zero field) against the nodes (finite field B).  On the reference first,
    then the same figures on the device."""
    refs = {m: reference(f"two-doors-{m}") for m in (9, 10, 17)}
    fig = {m: two_doors_figures(refs[m]) for m in refs}
    print(f"[two doors] (cells with roadmap, reachable nodes, largest finite field B) at min_dist2 9 / 10 / 17: {fig[9]} / {fig[10]} / {fig[17]}")
    assert fig[9][0] == fig[9][1] > 0 and fig[10][0] == fig[10][1] > 0, "every node reachable at 9 and at 10"
    narrow = (slice(9, 15), slice(19, 21))                              # what the 3 x 3 dilation leaves of the wall: columns 19 and 20
    assert refs[9].roadmap[narrow].any() and not refs[10].roadmap[narrow].any(), "the narrow door's roadmap is cut at 10"
    assert fig[10][2] > fig[9][2], "the way round is longer"
    assert 0 < fig[17][1] < fig[17][0], "some nodes reachable, some not, at 17"
    for m in refs:
        rm = case_checked(device, f"two-doors-{m}")
        zeros = torch.zeros_like(rm.field_entry)
        _, _, _, cells = RM.roadmap_nodes(rm.roadmap, rm.dist2, zeros, 8)
        f = n(rm.field_entry)
        assert (int(cells.item()), rm.K, int(f[f != INF].max())) == fig[m]


@guarded
def check_serpentine(device):
    """96 x 96 serpentine corridor: the field equals Dijkstra's and the round count stays below the number of mask pixels"""
    mask = serpentine()
    seed = (3, 3)
    ref, _ = ref_geodesic(mask, seed)
    assert (ref[mask != 0] != INF).all() and int(ref.max(initial=0, where=ref != INF)) > 12 * 96 * 4, "one long connected corridor"
    field, rounds = RM.grid_geodesic(t(mask, device), seed, return_rounds=True)
    print(f"[serpentine] {int(mask.sum())} mask pixels, longest way {int(ref[ref != INF].max())}, {rounds} relaxation rounds")
    assert np.array_equal(n(field), ref)
    assert 9 <= rounds < int(mask.sum()), "the way crosses the nine tiles many times, within the bound"


@guarded
def check_repeatable(device):
    """two calls on the same input give the same bytes, output by output"""
    cs = case("67x130")
    maps = types.SimpleNamespace(free_map_binary=t(cs.free, device), visible_map_binary=t(cs.unseen, device))
    a = RM.plan_roadmap(maps, cs.agent, 2.0, cs.cell)
    b = RM.plan_roadmap(maps, cs.agent, 2.0, cs.cell)
    for key in ("trav", "dist2", "feature", "roadmap", "field_agent", "field_entry", "node_rc", "node_dist2", "node_field"):
        x, y = n(getattr(a, key)), n(getattr(b, key))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key
    assert (a.K, a.entry_rc, a.entry_field, a.status, a.rounds) == (b.K, b.entry_rc, b.entry_field, b.status, b.rounds)
    assert n(a.path_to(a.K - 1)).tobytes() == n(b.path_to(b.K - 1)).tobytes()


@guarded
def check_status_bits(device):
    """an agent on an obstacle: empty map, bit 0; a seed outside the mask (or the image): all-unreachable field, bit 1"""
    cs = case("48x40")
    wall = (0, 0)                                                      # (the border is three pixels: the dilation does not reach row 0)
    assert not reference("48x40").trav[wall]
    status = torch.zeros(1, dtype=torch.int32, device=device)
    trav = RM.traversable_map(t(cs.free, device), t(cs.unseen, device), (0, 0), status=status)
    assert int(status.item()) == RM.STATUS_AGENT_OFF_MAP and not n(trav).any()
    status.zero_()
    RM.traversable_map(t(cs.free, device), t(cs.unseen, device), cs.agent, status=status)
    assert int(status.item()) == 0
    mask = t(reference("48x40").trav, device)
    for seed in (wall, (-1, 3), (3, 40)):
        status.zero_()
        field, rounds = RM.grid_geodesic(mask, seed, status=status, return_rounds=True)
        assert int(status.item()) == RM.STATUS_SEED_OFF_MASK and rounds == 0 and (n(field) == INF).all()
    status.zero_()
    RM.grid_geodesic(mask, cs.agent, status=status)
    assert int(status.item()) == 0
    maps = types.SimpleNamespace(free_map_binary=t(cs.free, device), visible_map_binary=t(cs.unseen, device))
    rm = RM.plan_roadmap(maps, wall, 2.0, 8)
    assert rm.status == (RM.STATUS_AGENT_OFF_MAP | RM.STATUS_SEED_OFF_MASK | RM.STATUS_NO_ENTRY) and rm.K == 0 and rm.entry_rc == (-1, -1)


@guarded
def check_refusals(device):
    """wrong dtype, shape or arguments raise in Python; the C entry points refuse what they name, before any launch"""
    cs = case("48x40")
    free, unseen = t(cs.free, device), t(cs.unseen, device)
    with pytest.raises(ValueError, match="dilate must be odd"):
        RM.traversable_map(free, unseen, cs.agent, dilate=4)
    with pytest.raises(ValueError, match="open_size"):
        RM.traversable_map(free, unseen, cs.agent, open_size=0)
    with pytest.raises(ValueError, match="uint8"):
        RM.traversable_map(free.to(torch.int32), unseen, cs.agent)
    with pytest.raises(ValueError, match="shape"):
        RM.traversable_map(free, unseen[:, :-1].contiguous(), cs.agent)
    with pytest.raises(ValueError, match="shape"):
        RM.traversable_map(free[0], unseen[0], cs.agent)
    with pytest.raises(ValueError, match="contiguous"):
        RM.traversable_map(free.t(), unseen.t(), cs.agent)
    with pytest.raises(ValueError, match="outside"):
        RM.traversable_map(free, unseen, (48, 0))
    with pytest.raises(TypeError):
        RM.clearance_field(cs.free)
    dist2, feature = RM.clearance_field(free)
    with pytest.raises(ValueError, match="int32"):
        RM.voronoi_roadmap(free, dist2.to(torch.int64), feature, 4)
    with pytest.raises(ValueError, match="shape"):
        RM.voronoi_roadmap(free, dist2, feature[..., :1].contiguous(), 4)
    with pytest.raises(ValueError, match="min_dist2"):
        RM.voronoi_roadmap(free, dist2, feature, -1)
    with pytest.raises(ValueError, match="cell"):
        RM.roadmap_nodes(free, dist2, dist2, 0)
    with pytest.raises(ValueError, match="cell"):
        RM.roadmap_nodes(free, dist2, dist2, 65)
    with pytest.raises(ValueError, match="capacity"):
        RM.trace_path(free, dist2, (5, 5), -1)
    lib, st = _lib.get(), _lib.stream_ptr(torch.device(device))
    H, W = cs.free.shape
    scratch = torch.empty(int(lib.gs_roadmap_scratch_bytes(H, W)), dtype=torch.uint8, device=device)
    word = torch.zeros(4, dtype=torch.int32, device=device)
    out = torch.zeros(H, W, dtype=torch.uint8, device=device)
    p = R._ptr
    assert lib.gs_roadmap_scratch_bytes(0, 5) == 0 and lib.gs_roadmap_scratch_bytes(5, 4097) == 0 and lib.gs_roadmap_scratch_bytes(4096, 4096) > 0
    for bad in (dict(dilate=2), dict(dilate=17), dict(open_size=17), dict(H=0), dict(W=4097), dict(agent_r=H), dict(agent_c=-1), dict(free=None),
                dict(scratch=None), dict(status=None)):
        a = dict(H=H, W=W, free=p(free), unseen=p(unseen), agent_r=5, agent_c=5, open_size=4, dilate=3, trav=p(out), scratch=p(scratch), status=p(word))
        a.update(bad)
        assert lib.gs_traversable_map(a["H"], a["W"], a["free"], a["unseen"], a["agent_r"], a["agent_c"], a["open_size"], a["dilate"], a["trav"],
                                      a["scratch"], a["status"], st) == GS_EINVAL, bad
    assert lib.gs_clearance_field(H, W, None, p(dist2), p(feature), p(scratch), st) == GS_EINVAL
    assert lib.gs_clearance_field(H, 0, p(free), p(dist2), p(feature), p(scratch), st) == GS_EINVAL
    assert lib.gs_voronoi_roadmap(H, W, p(free), p(dist2), p(feature), -1, 4, p(out), st) == GS_EINVAL
    assert lib.gs_voronoi_roadmap(H, W, p(free), p(dist2), p(feature), 4, -1, p(out), st) == GS_EINVAL
    import ctypes as C
    rounds = C.c_int32(7)
    assert lib.gs_grid_geodesic(H, W, p(free), 5, 5, None, None, p(scratch), p(word), C.byref(rounds), st) == GS_EINVAL
    assert lib.gs_grid_geodesic(4097, W, p(free), 5, 5, None, p(dist2), p(scratch), p(word), C.byref(rounds), st) == GS_EINVAL
    assert lib.gs_roadmap_entry(H, W, p(free), None, p(word), p(scratch), st) == GS_EINVAL
    assert lib.gs_roadmap_entry(H, W, p(free), p(dist2), p(word), None, st) == GS_EINVAL
    assert lib.gs_roadmap_nodes(H, W, p(free), p(dist2), p(dist2), 0, p(word), p(word), p(word), p(word), p(scratch), st) == GS_EINVAL
    assert lib.gs_roadmap_nodes(H, W, p(free), p(dist2), p(dist2), 65, p(word), p(word), p(word), p(word), p(scratch), st) == GS_EINVAL
    assert lib.gs_trace_path(H, W, p(free), p(dist2), 5, 5, None, -1, p(word), p(word), st) == GS_EINVAL
    assert lib.gs_trace_path(H, W, p(free), p(dist2), 5, 5, None, 4, None, p(word), st) == GS_EINVAL
    assert "gs_trace_path" in _lib.get().gs_last_error().decode()
    assert not n(out).any() and not n(word).any() and rounds.value == 7, "nothing was launched"


def check_pixel_world_round_trip():
    """pixel_to_world is the inverse of world_to_pixel (host and tensor forms), for an odd and an even grid and an off-centre world"""
    for grid in ((64, 48), (67, 131)):
        kw = dict(world_center=(0.3, -0.2), world_shape=(8.0, 6.5), grid_shape=grid, height=1000.0)
        rc = np.stack(np.meshgrid(np.arange(grid[1]), np.arange(grid[0]), indexing="ij"), -1).reshape(-1, 2)
        xz = RM.pixel_to_world(rc, **kw)
        assert np.abs(RM.world_to_pixel(xz, **kw) - rc).max() < 1e-9
        assert np.array_equal(np.rint(RM.world_to_pixel(xz, **kw)).astype(np.int64), rc)
        assert np.abs(n(RM.pixel_to_world(torch.from_numpy(rc), **kw)).astype(np.float64) - xz).max() < 1e-5
    # the x axis runs along the columns, the z axis against the rows, one pixel = world extent / grid size
    a, b = RM.pixel_to_world(np.array([[10, 20], [11, 22]]), (0.0, 0.0), (8.0, 6.0), (64, 48))
    assert np.allclose(b - a, [2 * 8.0 / 64, -6.0 / 48])


# ---- GPU only: through the rasteriser ---------------------------------------------------------------------------------------------------------------

WORLD = dict(world_center=(0.5, -0.25), world_shape=(8.0, 6.0), grid_shape=(64, 48))
BAND = (0.1, 1.3)


def splat_room(device):
    """A few opaque Gaussians per pixel column: a grey floor under the whole 64 x 48 map (below the height band: seen, free) and a wall in the
    band, 5 pixels thick at columns 30..34, with a door at rows 20..29 -> (params, wall mask [48, 64])"""
    W, H = WORLD["grid_shape"]
    rc = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), -1).reshape(-1, 2)
    xz = RM.pixel_to_world(rc, **WORLD)
    wall = np.zeros((H, W), bool)
    wall[:, 30:35] = True
    wall[20:30, 30:35] = False
    wxz = xz[wall.reshape(-1)]
    means = np.concatenate([np.stack([xz[:, 0], np.zeros(len(xz)), xz[:, 1]], 1), np.stack([wxz[:, 0], np.full(len(wxz), -0.7), wxz[:, 1]], 1)])
    P = len(means)
    colors = np.concatenate([np.full((len(xz), 3), 0.5), np.tile([[0.8, 0.2, 0.2]], (len(wxz), 1))])
    params = dict(means3D=means, rgb_colors=colors, unnorm_rotations=np.tile([[1.0, 0.0, 0.0, 0.0]], (P, 1)),
                  logit_opacities=np.full((P, 1), 8.0), log_scales=np.full((P, 1), np.log(0.02)))
    return {k: torch.tensor(v, dtype=torch.float32, device=device).contiguous() for k, v in params.items()}, wall


def mapper_of(params, device, W=64, H=48):
    from activesplat_amd import synthetic as syn
    from activesplat_amd.mapper import SplatMapper
    mp = SplatMapper(syn.intrinsics(W, H), W, H, device=device)
    mp.params = params
    return mp


@guarded
def check_gaussian_lands_on_its_pixel(device):
    """one Gaussian at the world position of a pixel's sample point is seen at that pixel, and world_to_pixel names it"""
    from activesplat_amd import topdown as TD
    W, H = WORLD["grid_shape"]
    for rc in ((7, 9), (40, 63), (0, 0), (24, 32)):
        x, z = RM.pixel_to_world(np.array(rc), **WORLD)
        assert tuple(np.rint(RM.world_to_pixel((x, z), **WORLD)).astype(int)) == rc
        params = dict(means3D=[[x, 0.0, z]], rgb_colors=[[0.2, 0.4, 0.6]], unnorm_rotations=[[1.0, 0.0, 0.0, 0.0]], logit_opacities=[[8.0]],
                      log_scales=[[float(np.log(0.02))]])
        params = {k: torch.tensor(v, dtype=torch.float32, device=device) for k, v in params.items()}
        maps = TD.topdown_maps(params, TD.topdown_camera(device=device, **WORLD), *BAND, scale_modifier=1.0)
        seen = n(maps.visible_map_binary) == 0
        rgb = n(maps.visible_rgb).astype(np.int64)
        dark = np.unravel_index(int(np.argmin(rgb.sum(-1))), (H, W))
        assert seen[rc] and tuple(int(v) for v in dark) == rc, (rc, dark, int(seen.sum()))
        off = RM.pixel_to_world(np.array(rc) + [0, 1], **WORLD)
        assert tuple(np.rint(RM.world_to_pixel(off, **WORLD)).astype(int)) == (rc[0], rc[1] + 1)


@guarded
def check_mapper_plan_step(device):
    """a floor and a wall with a door as Gaussians -> SplatMapper.roadmap, then plan_step: the traversable map is scipy's of the drawn wall,
    the waypoints start at the agent's pixel, end at a node and stay on traversable pixels"""
    params, wall = splat_room(device)
    mp = mapper_of(params, device)
    agent_rc = (24, 10)
    ax, az = RM.pixel_to_world(np.array(agent_rc), **WORLD)
    rm, positions = mp.roadmap(upper=BAND[0], lower=BAND[1], agent_xz=(ax, az), agent_radius=0.25, node_spacing=1.0, node_y=-0.5, scale_modifier=1.0, **WORLD)
    trav = n(rm.trav)
    want, st = ref_traversable((~wall).astype(np.uint8), np.zeros_like(wall, np.uint8), agent_rc, 4, 3)
    assert st == 0 and np.array_equal(trav, want), "the rendered free map is the floor without the wall"
    assert rm.agent_rc == agent_rc and rm.cell == 8 and rm.min_dist2 == 4 and rm.status == 0 and rm.K >= 4
    assert isinstance(positions, np.ndarray) and positions.shape == (rm.K, 3) and positions.dtype == np.float64
    back = np.rint(RM.world_to_pixel(positions[:, [0, 2]], **WORLD)).astype(np.int32)
    assert np.array_equal(back, n(rm.node_rc)) and (positions[:, 1] == -0.5).all()
    assert (n(rm.node_rc)[:, 1] > 34).any(), "nodes beyond the door"
    c2w = np.eye(4)
    c2w[:3, 3] = [ax, -0.5, az]
    step = mp.plan_step(torch.tensor(c2w, dtype=torch.float32), upper=BAND[0], lower=BAND[1], agent_radius=0.25, node_spacing=1.0, scale_modifier=1.0, **WORLD)
    inv, node, path = step["invisibility"], step["node"], n(step["path_rc"])
    assert np.array_equal(n(step["roadmap"].node_rc), n(rm.node_rc)) and len(inv) == rm.K and 0 <= node < rm.K
    length = n(rm.node_path_length())
    assert node == min(range(rm.K), key=lambda k: (-inv[k], length[k], k)), "largest invisibility, then the shorter way, then the lower index"
    assert tuple(path[0]) == agent_rc and tuple(path[-1]) == tuple(n(rm.node_rc)[node])
    assert path_weight(path, trav)[0] == length[node]
    way = n(step["waypoints"])
    assert way.shape == (len(path), 3) and (way[:, 1] == -0.5).all()
    assert np.array_equal(np.rint(RM.world_to_pixel(way[:, [0, 2]].astype(np.float64), **WORLD)).astype(np.int32), path)
