"""Shared checks of the simulated agent (activesplat_amd/agent.py, activesplat_amd/explore.py; gs_mesh_navgrid): run on the host-emulated kernels by
tests/test_agent.py and on the MI355X by tests/test_gpu_agent.py.

Expected values
* `restate_ranges` + `restate_bits`: the rule of include/gsplat_hip.h (gs_mesh_navgrid) in numpy float64, written from the rule's text: every
  triangle against every cell, stage after stage Sutherland-Hodgman with the polygon stored (vectorised over the cells of one triangle; numpy's
  elementwise float64 operations are rounded one by one, as the rule asks).  No bounding box, no tile, no pre-sorting: nothing of the kernel's
  structure.  Every grid comparison is EXACT (array_equal).
* `check_reference_conditions`: exactness means something only if no cell of a random case hangs on a rounding.  For every random case the
  restatement alone is evaluated with all cell borders moved outward and inward by 1e-7 m and with the height thresholds raised and lowered by
  1e-7 m (once the two obstacle thresholds, once all three): every variant gives the same grid.  No cell is skipped or masked.
* the dyadic room: all coordinates are multiples of 1/16 m and lie ON cell borders, so touching is decided by exact comparisons of exact numbers;
  a few named cells are also written out by hand (HAND_CELLS).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from activesplat_amd import _lib
from activesplat_amd import agent as AG
from activesplat_amd import explore as EX
from activesplat_amd import rasterizer as R
from activesplat_amd import sensor as S
from tests import mesh_cases as mc

GS_EINVAL = 1
FLOOR_Y, CLIMB, HEIGHT = 0.0, 0.2, 1.5
GRID = dict(origin_xz=(-1.5, -1.25), cell=0.0625, grid_shape=(40, 48))          # 40 x 48 cells: partial tiles in both directions
SOUP_SEEDS = (0, 1, 2)

# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------------


def _clip_stage(poly, cnt, k, bound, keep_ge):
    """one Sutherland-Hodgman stage on N polygons at once: poly [N, 8, 3], cnt [N]; coordinate k against bound [N]"""
    N = len(cnt)
    out, m = np.zeros_like(poly), np.zeros(N, np.int64)
    rows = np.arange(N)
    inside = (lambda p: p[:, k] >= bound) if keep_ge else (lambda p: p[:, k] <= bound)
    for i in range(int(cnt.max(initial=0))):
        act = i < cnt
        a = poly[:, i]
        b = poly[rows, np.where(i + 1 < cnt, i + 1, 0)]
        ina, inb = inside(a), inside(b)
        emit = act & ina
        out[rows[emit], m[emit]] = a[emit]
        m[emit] += 1
        cross = act & (ina != inb)
        with np.errstate(all="ignore"):
            t = (bound - a[:, k]) / (b[:, k] - a[:, k])
            p = a + t[:, None] * (b - a)
        p[:, k] = bound
        out[rows[cross], m[cross]] = p[cross]
        m[cross] += 1
    return out, m


def restate_ranges(vertices, triangles, origin_xz, cell, grid_shape, shift=0.0):
    """per triangle: None (dropped: an index outside the vertices, a non-finite vertex) or (lo [H, W], hi [H, W], Ylo, Yhi): the y range of the
    clipped polygon in every cell (+inf, -inf where it is empty) and of the triangle itself.  shift: every cell border moved outward by it."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    H, W = grid_shape
    x0, z0, cell = np.float64(origin_xz[0]), np.float64(origin_xz[1]), np.float64(cell)
    cols, rows = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    xa, xb = (x0 + cols * cell) - shift, (x0 + (cols + 1.0) * cell) + shift
    za, zb = (z0 + rows * cell) - shift, (z0 + (rows + 1.0) * cell) + shift
    XA, XB = np.tile(xa, H), np.tile(xb, H)
    ZA, ZB = np.repeat(za, W), np.repeat(zb, W)
    N = H * W
    out = []
    for t in tri:
        if (t < 0).any() or (t >= len(v32)).any():
            out.append(None)
            continue
        p = v32[t].astype(np.float64)
        if not np.isfinite(p).all():
            out.append(None)
            continue
        poly = np.zeros((N, 8, 3))
        poly[:, :3] = p[None]
        cnt = np.full(N, 3, np.int64)
        for k, bound, ge in ((0, XA, True), (0, XB, False), (2, ZA, True), (2, ZB, False)):
            poly, cnt = _clip_stage(poly, cnt, k, bound, ge)
        valid = np.arange(8)[None, :] < cnt[:, None]
        lo = np.where(valid, poly[:, :, 1], np.inf).min(1).reshape(H, W)
        hi = np.where(valid, poly[:, :, 1], -np.inf).max(1).reshape(H, W)
        out.append((lo, hi, p[:, 1].min(), p[:, 1].max()))
    return out


def _bits(lo, hi, y_floor, y_step, y_head):
    return ((hi >= y_floor) & (lo <= y_step)).astype(np.uint8) | (((hi > y_step) & (lo < y_head)).astype(np.uint8) << 1)


def restate_bits(ranges, grid_shape, floor_y=FLOOR_Y, max_climb=CLIMB, agent_height=HEIGHT, raise_obstacle=0.0, raise_floor=0.0):
    """the grid of the rule from `restate_ranges`; raise_*: added to the thresholds (floor_y + max_climb and floor_y + agent_height; floor_y - max_climb)"""
    f = np.float64
    y_floor = (f(floor_y) - f(max_climb)) + raise_floor
    y_step, y_head = (f(floor_y) + f(max_climb)) + raise_obstacle, (f(floor_y) + f(agent_height)) + raise_obstacle
    grid = np.zeros(grid_shape, np.uint8)
    for r in ranges:
        if r is None:
            continue
        lo, hi, ylo, yhi = r
        if int(_bits(np.array(ylo), np.array(yhi), y_floor, y_step, y_head)) == 0:      # the pre-test, per triangle, first
            continue
        grid |= _bits(lo, hi, y_floor, y_step, y_head)       # (an empty polygon has lo = +inf, hi = -inf: both tests fail)
    return grid


def restate(vertices, triangles, origin_xz, cell, grid_shape, floor_y=FLOOR_Y, max_climb=CLIMB, agent_height=HEIGHT):
    return restate_bits(restate_ranges(vertices, triangles, origin_xz, cell, grid_shape), grid_shape, floor_y, max_climb, agent_height)

# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------


def soup(seed, n=60):
    """n random triangles: centres uniform in [-1.2, 1.2] x [-0.4, 2.0] x [-1.5, 1.5], each vertex the centre plus uniform +-0.35, as fp32"""
    rng = np.random.RandomState(seed)
    centres = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.4, 2.0, n), rng.uniform(-1.5, 1.5, n)], 1)
    v = (centres[:, None, :] + rng.uniform(-0.35, 0.35, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def quad(a, b, c, d):
    return np.array([a, b, c, d], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def room_parts(x=(-1.25, 1.25), z=(-1.0, 1.0), top=2.5, door=None):
    """a floor of two triangles and four walls from the floor to `top` (vertical triangles); door = (z_lo, z_hi): a gap in the wall at x[1]"""
    (xl, xh), (zl, zh) = x, z
    parts = [quad((xl, 0, zl), (xh, 0, zl), (xh, 0, zh), (xl, 0, zh)),
             quad((xl, 0, zl), (xl, top, zl), (xl, top, zh), (xl, 0, zh)),
             quad((xl, 0, zl), (xh, 0, zl), (xh, top, zl), (xl, top, zl)),
             quad((xl, 0, zh), (xh, 0, zh), (xh, top, zh), (xl, top, zh))]
    spans = [(zl, zh)] if door is None else [(zl, door[0]), (door[1], zh)]
    parts += [quad((xh, 0, a), (xh, top, a), (xh, top, b), (xh, 0, b)) for a, b in spans]
    return parts


def dyadic_room():
    """every coordinate a multiple of 1/16 m, on the cell borders of GRID: a floor of two triangles, four walls, a pillar, a 0.125 m step (stays
    floor), a table top at 0.75 m (an obstacle) and a lintel at 2.0 m (neither)"""
    parts = room_parts()
    parts.append(mc.box(((0.5, 0.75), (0.0, 2.5), (0.25, 0.5))))                                   # pillar
    parts.append(mc.box(((-1.0, -0.5), (0.0, 0.125), (-0.75, -0.25))))                             # step
    parts.append(quad((-0.5, 0.75, 0.25), (0.0, 0.75, 0.25), (0.0, 0.75, 0.75), (-0.5, 0.75, 0.75)))   # table top
    parts.append(quad((0.0, 2.0, -0.75), (0.5, 2.0, -0.75), (0.5, 2.0, -0.5), (0.0, 2.0, -0.5)))       # lintel
    return mc.merge(parts)


# (r, c) -> value, worked out by hand from the closed-square rule.  Column c spans x in [-1.5 + c / 16, -1.5 + (c + 1) / 16], row r spans z in
# [-1.25 + r / 16, -1.25 + (r + 1) / 16].  The wall at x = -1.25 is the border of columns 3 and 4: both touch it and are blocked (3: the floor's
# edge touches too); column 2 touches nothing.  The step covers columns 8..15, rows 8..15 and never rises above the climb.  The table top covers
# columns 16..23, rows 24..31 and touches the ring around them, corner cells included.  The lintel (columns 24..31, rows 8..11) is above the head.
# The pillar's four sides run along the borders of columns 32..35, rows 24..27: the cells on both sides of each side are blocked, corner cells
# included; the pillar is hollow, so the four cells strictly inside it (rows 25..26, columns 33..34) see only its bottom: floor.
HAND_CELLS = {(0, 0): 0, (20, 2): 0, (20, 3): 3, (20, 4): 3, (20, 5): 1, (12, 12): 1, (7, 7): 1, (28, 20): 3, (23, 15): 3, (22, 14): 1,
              (10, 28): 1, (24, 32): 3, (25, 33): 1, (23, 31): 3, (28, 36): 3, (22, 30): 1, (3, 20): 3, (4, 20): 3, (2, 20): 0, (36, 20): 3, (37, 20): 0}


def two_rooms():
    """two dyadic rooms joined by a door (0.5 m wide) in the wall they share -> (vertices, triangles, colours)"""
    parts = room_parts(x=(-1.25, 0.0), z=(-0.75, 0.75), top=2.0, door=(-0.25, 0.25))
    parts += room_parts(x=(0.0, 1.25), z=(-0.75, 0.75), top=2.0)[:1] + room_parts(x=(0.0, 1.25), z=(-0.75, 0.75), top=2.0)[2:]
    for xl, xh in ((-1.25, 0.0), (0.0, 1.25)):                                                     # ceilings, so that every ray ends on the mesh
        parts.append(quad((xl, 2.0, -0.75), (xh, 2.0, -0.75), (xh, 2.0, 0.75), (xl, 2.0, 0.75)))
    v, t = mc.merge(parts)
    return v, t, np.random.RandomState(7).randint(40, 256, (len(v), 3)).astype(np.uint8)


_cache = {}


def reference(name):
    """(mesh, the restated grid) of a named case, computed once per session and left unchanged"""
    if name not in _cache:
        mesh = soup(int(name[4:])) if name.startswith("soup") else dyadic_room()
        grid = restate(*mesh, **GRID)
        grid.setflags(write=False)
        _cache[name] = (mesh, grid)
    return _cache[name]


def check_reference_conditions():
    H, W = GRID["grid_shape"]
    for seed in SOUP_SEEDS:
        mesh, base = reference(f"soup{seed}")
        assert set(np.unique(base).tolist()) == {0, 1, 2, 3}, (seed, "all four cell values are present")
        ranges = restate_ranges(*mesh, **GRID)
        assert np.array_equal(restate_bits(ranges, (H, W)), base)
        for d in (1e-7, -1e-7):
            moved = restate_bits(restate_ranges(*mesh, shift=d, **GRID), (H, W))
            assert np.array_equal(moved, base), (seed, "cell borders moved by", d, int((moved != base).sum()))
            for kw in (dict(raise_obstacle=d), dict(raise_obstacle=d, raise_floor=d)):
                moved = restate_bits(ranges, (H, W), **kw)
                assert np.array_equal(moved, base), (seed, "thresholds moved by", kw, int((moved != base).sum()))
    mesh, room = reference("room")
    for rc, want in HAND_CELLS.items():
        assert room[rc] == want, (rc, int(room[rc]), want)
    # the room as a whole: void outside the walls, floor or blocked inside, nothing else
    assert (room[:, :3] == 0).all() and (room[:, 45:] == 0).all() and (room[:3] == 0).all() and (room[37:] == 0).all()
    assert (room[3:37, 3:45] != 0).all() and (room[5:35, 5:7] == 1).all()

# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------


def n(t):
    return t.detach().cpu().numpy()


def scene_of(mesh, device):
    return S.MeshScene(mesh[0], mesh[1], device=device)


def raw_scene(vertices, triangles, device):
    """a MeshScene whose triangles were NOT validated (MeshScene refuses an index outside the vertices; the kernel has to drop it)"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    good = S.MeshScene(v if len(v) else np.zeros((1, 3), np.float32), np.zeros((0, 3), np.int32), device=device)
    good.vertices = torch.from_numpy(np.ascontiguousarray(v)).to(device)
    good.triangles = torch.from_numpy(np.ascontiguousarray(np.asarray(triangles, np.int32).reshape(-1, 3))).to(device)
    return good


def run(device, mesh, scene=None, **over):
    kw = dict(GRID, floor_y=FLOOR_Y, agent_height=HEIGHT, max_climb=CLIMB)
    kw.update(over)
    grid = AG.navgrid(scene if scene is not None else scene_of(mesh, device), **kw)
    assert grid.dtype == torch.uint8 and tuple(grid.shape) == tuple(kw["grid_shape"]) and grid.device.type == torch.device(device).type
    return n(grid)


def check_soup(device, seed):
    mesh, want = reference(f"soup{seed}")
    got = run(device, mesh)
    assert np.array_equal(got, want), (seed, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())


def check_room(device):
    mesh, want = reference("room")
    scene = scene_of(mesh, device)
    got = run(device, mesh, scene)
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    for rc, value in HAND_CELLS.items():
        assert got[rc] == value, (rc, int(got[rc]), value)
    need, longest = scene.last_navgrid_counts
    assert longest >= 2 and need >= 2 * 9, "the two floor triangles are in the list of each of the 3 x 3 tiles"


def check_odd_sizes(device):
    room, _ = reference("room")
    v, t = room
    # a 1 x 1 grid and a 17 x 16 grid (one full tile and one row more), at origins that cut through the room's furniture
    for shape, origin in (((1, 1), (0.5, 0.25)), ((1, 1), (-1.375, 0.0)), ((17, 16), (-0.5, -0.25)), ((16, 17), (0.0, 0.0))):
        kw = dict(origin_xz=origin, cell=0.0625, grid_shape=shape)
        got = run(device, room, **kw)
        assert np.array_equal(got, restate(v, t, **kw)), (shape, origin)
    assert run(device, room, origin_xz=(0.5, 0.25), cell=0.0625, grid_shape=(1, 1))[0, 0] == 3       # a cell of the pillar
    assert run(device, room, origin_xz=(-1.375, 0.0), cell=0.0625, grid_shape=(1, 1))[0, 0] == 0     # outside the wall
    # a mesh entirely outside the grid, and no mesh at all
    far = (v + np.array([50.0, 0.0, -30.0], np.float32), t)
    assert (run(device, far) == 0).all() and (restate(*far, **GRID) == 0).all()
    assert (run(device, (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))) == 0).all()
    # a triangle with an index outside the vertices, one with a NaN vertex and one with an infinite vertex next to valid ones: dropped
    sv, st = soup(0)
    bad_t = np.concatenate([np.array([[0, 1, len(sv) + 5], [2, -1, 3]], np.int32), st, np.array([[len(sv), len(sv) + 1, len(sv) + 2],
                                                                                                [3, 4, len(sv) + 3]], np.int32)])
    bad_v = np.concatenate([sv, np.array([[0.0, 0.1, 0.0], [np.nan, 0.1, 0.2], [0.3, 0.1, -0.2], [0.1, np.inf, 0.1]], np.float32)])
    got = run(device, None, raw_scene(bad_v, bad_t, device))
    assert np.array_equal(got, reference("soup0")[1]) and np.array_equal(restate(bad_v, bad_t, **GRID), reference("soup0")[1])
    # zero-area triangles: three equal vertices (a point on the floor), and three collinear ones (a rod through the head band)
    zv = np.array([[0.03, 0.0, 0.03], [0.03, 0.0, 0.03], [0.03, 0.0, 0.03], [-0.4, 1.0, -0.4], [0.0, 1.0, 0.0], [0.2, 1.0, 0.2]], np.float32)
    zt = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    got, want = run(device, (zv, zt)), restate(zv, zt, **GRID)
    assert np.array_equal(got, want) and got[20, 24] == 3 and (got == 1).sum() == 0 and (got == 2).sum() >= 8


def _abi_call(device, scene, capacity, guard=4096, **over):
    """gs_mesh_navgrid with a scratch of exactly the layout's size and a grid of exactly H x W bytes, both between canary bytes ->
    (rc, grid, counts, canaries intact, layout)"""
    lib = _lib.get()
    H, W = over.pop("grid_shape", GRID["grid_shape"])
    T = scene.num_triangles
    layout = _lib.GsMeshLayout()
    assert lib.gs_mesh_navgrid_layout(T, W, H, capacity, C.byref(layout)) == 0
    nbytes = int(layout.total_bytes)
    assert nbytes % 16 == 0 and guard % 16 == 0
    buf = torch.full((guard + nbytes + guard,), 0xAB, dtype=torch.uint8, device=device)
    out = torch.full((guard + H * W + guard,), 0xCD, dtype=torch.uint8, device=device)
    counts = torch.zeros(2, dtype=torch.int32, device=device)
    a = dict(num_vertices=scene.num_vertices, vertices=R._ptr(scene.vertices), num_triangles=T, triangles=R._ptr(scene.triangles),
             x0=GRID["origin_xz"][0], z0=GRID["origin_xz"][1], cell=GRID["cell"], floor_y=FLOOR_Y, max_climb=CLIMB, agent_height=HEIGHT, width=W, height=H,
             scratch=C.c_void_p(buf.data_ptr() + guard), capacity=capacity, grid=C.c_void_p(out.data_ptr() + guard), counts=R._ptr(counts))
    a.update(over)
    rc = lib.gs_mesh_navgrid(a["num_vertices"], a["vertices"], a["num_triangles"], a["triangles"], a["x0"], a["z0"], a["cell"], a["floor_y"], a["max_climb"],
                             a["agent_height"], a["width"], a["height"], a["scratch"], a["capacity"], a["grid"], a["counts"], _lib.stream_ptr(torch.device(device)))
    intact = bool((buf[:guard] == 0xAB).all() and (buf[guard + nbytes:] == 0xAB).all() and (out[:guard] == 0xCD).all() and (out[guard + H * W:] == 0xCD).all())
    return rc, n(out[guard:guard + H * W]).reshape(H, W).copy(), [int(x) & 0xffffffff for x in counts.tolist()], intact, layout


def check_capacity_and_guards(device):
    mesh, want = reference("soup0")
    scene = scene_of(mesh, device)
    rc, grid, (need, longest), intact, layout = _abi_call(device, scene, capacity=1)
    assert rc == 0 and intact and need > 9 and need >= longest >= (need + 8) // 9
    assert int(layout.total_bytes) >= int(layout.list) + 4 and int(layout.records) >= 256 and int(layout.rects) - int(layout.records) >= 48 * scene.num_triangles
    assert (grid == 0).all(), "a launch whose lists did not fit leaves a cleared grid"
    rc, grid, (need2, longest2), intact, _ = _abi_call(device, scene, capacity=need)
    assert rc == 0 and intact and (need2, longest2) == (need, longest) and np.array_equal(grid, want)
    rc, grid, _, intact, _ = _abi_call(device, scene, capacity=need - 1)
    assert rc == 0 and intact and (grid == 0).all()
    # navgrid starting from capacity 1 returns the roomy result and remembers what was needed
    H, W = GRID["grid_shape"]
    scene.capacities[("navgrid", H, W)] = 1
    assert np.array_equal(run(device, mesh, scene), want)
    assert scene.capacities[("navgrid", H, W)] >= need and scene.last_navgrid_counts == (need, longest)
    # the room: the canaries around a 17 x 16 grid (partial tiles) stay intact as well
    room, _ = reference("room")
    rc, grid, _, intact, _ = _abi_call(device, scene_of(room, device), capacity=4096, grid_shape=(17, 16))
    assert rc == 0 and intact and np.array_equal(grid, restate(*room, GRID["origin_xz"], GRID["cell"], (17, 16)))


def check_repeatable(device):
    for name in ("soup1", "room"):
        mesh, want = reference(name)
        a, b = run(device, mesh), run(device, mesh)
        assert a.tobytes() == b.tobytes()
        v, t = mesh
        assert np.array_equal(run(device, (v, t[::-1].copy())), a) and np.array_equal(run(device, (v, t[:, [1, 2, 0]].copy())), want)


def check_refusals(device):
    lib = _lib.get()
    scene = scene_of(reference("room")[0], device)

    def call(**over):
        rc, grid, _, intact, _ = _abi_call(device, scene, 4096, **over)
        return rc, grid, intact
    rc, grid, intact = call()
    assert rc == 0 and intact and (grid != 0xCD).all()                                              # (the call itself is well formed)
    inf, nan = float("inf"), float("nan")
    for over, text in ((dict(vertices=None), b"null"), (dict(triangles=None), b"null"), (dict(scratch=None), b"null"), (dict(grid=None), b"null"),
                       (dict(counts=None), b"null"), (dict(width=0), b"grid size"), (dict(height=0), b"grid size"), (dict(width=16385), b"grid size"),
                       (dict(height=16385), b"grid size"), (dict(num_triangles=-1), b"num_triangles"), (dict(num_vertices=-1), b"num_vertices"),
                       (dict(cell=0.0), b"cell"), (dict(cell=-1.0), b"cell"), (dict(cell=inf), b"cell"), (dict(cell=nan), b"cell"),
                       (dict(x0=nan), b"finite"), (dict(z0=inf), b"finite"), (dict(floor_y=-inf), b"finite"), (dict(max_climb=nan), b"finite"),
                       (dict(agent_height=inf), b"finite"), (dict(max_climb=-0.1), b"max_climb"), (dict(agent_height=0.2), b"agent_height"),
                       (dict(agent_height=0.1), b"agent_height")):
        rc, grid, intact = call(**over)
        assert rc == GS_EINVAL and text in lib.gs_last_error(), (over, lib.gs_last_error())
        assert intact and (grid == 0xCD).all(), over                                                # nothing was launched
    layout = _lib.GsMeshLayout()
    assert lib.gs_mesh_navgrid_layout(-1, 8, 8, 1, C.byref(layout)) == GS_EINVAL and lib.gs_mesh_navgrid_layout(1, 0, 8, 1, C.byref(layout)) == GS_EINVAL
    assert lib.gs_mesh_navgrid_layout(1, 8, 8, 1, None) == GS_EINVAL
    # num_triangles == 0 with null mesh arrays is valid and clears the grid
    rc, grid, intact = call(num_triangles=0, vertices=None, triangles=None)
    assert rc == 0 and intact and (grid == 0).all()
    # the binding's own checks
    with pytest.raises(TypeError, match="MeshScene"):
        AG.navgrid(None, **GRID, floor_y=0.0)
    for bad in (dict(cell=0.0), dict(cell=float("nan")), dict(grid_shape=(0, 4)), dict(grid_shape=(4, 16385)), dict(max_climb=-1.0), dict(agent_height=0.2),
                dict(floor_y=float("inf"))):
        with pytest.raises(ValueError):
            AG.navgrid(scene, **dict(dict(GRID, floor_y=0.0), **bad))


def check_no_cpu_fallback():
    _lib.unload_for_tests()
    v, t = reference("room")[0]
    scene = object.__new__(S.MeshScene)
    scene.device, scene.vertices, scene.triangles, scene.capacities = torch.device("cpu"), torch.from_numpy(v), torch.from_numpy(t), {}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AG.navgrid(scene, **GRID, floor_y=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AG.NavGrid.build(scene, **GRID, floor_y=0.0)

# ---- the agent (host logic) -----------------------------------------------------------------------------------------------------------------


def room_nav(device):
    return AG.NavGrid.build(scene_of(reference("room")[0], device), **GRID, floor_y=FLOOR_Y)


def check_navgrid_erosion(device):
    nav = room_nav(device)
    grid = reference("room")[1]
    assert np.array_equal(n(nav.grid), grid) and nav.free.dtype == bool and nav.free.shape == grid.shape
    # radius 0.1 m at 1/16 m cells: ceil(2.56) = 3, i.e. at least two cells from everything that is not floor
    from scipy import ndimage
    want = ndimage.distance_transform_edt(np.pad(grid == 1, 1)) [1:-1, 1:-1] ** 2 >= 3 - 1e-9
    assert np.array_equal(nav.free, want & (grid == 1))
    assert nav.is_free(-0.3, 0.0) and not nav.is_free(-1.2, 0.0) and not nav.is_free(5.0, 0.0) and not nav.is_free(0.6, 0.3)
    assert nav.cell_of(-1.5, -1.25) == (0, 0) and nav.cell_of(-1.5 - 1e-9, 1.25) == (40, -1)


def check_agent(device, tmp_path):
    nav = room_nav(device)
    agent = AG.SimAgent(nav, (-0.3, 0.0))
    assert agent.substeps == 5                                                   # ceil(0.065 / (0.0625 / 4))
    # a full circle returns the same pose bits, either way round; half a circle does not
    first = agent.X_WV
    assert np.array_equal(first[:3, :3], np.eye(3)) and first[:3, 3].tolist() == [-0.3, 1.25, 0.0]
    for _ in range(18):
        assert agent.step(AG.TURN_LEFT)
    assert not np.array_equal(agent.X_WV, first)
    for _ in range(18):
        agent.step(AG.TURN_LEFT)
    assert agent.X_WV.tobytes() == first.tobytes() and agent.heading_steps == 36
    for _ in range(36):
        agent.step(AG.TURN_RIGHT)
    assert agent.X_WV.tobytes() == first.tobytes()
    for a in (AG.LOOK_UP, AG.LOOK_DOWN, AG.LOOK_DOWN, AG.LOOK_UP, AG.STOP):
        agent.step(a)
    assert agent.X_WV.tobytes() == first.tobytes() and agent.path_length == 0.0 and len(agent.actions) == 77
    # the pitch is about the camera's x and is not clamped: seven tilts up is 105 degrees, the view direction points up and backwards
    for _ in range(7):
        agent.step(AG.LOOK_UP)
    view = agent.X_WV[:3, :3] @ np.array([0.0, 0.0, -1.0])
    assert np.allclose(view, [0.0, np.sin(np.radians(105.0)), -np.cos(np.radians(105.0))], atol=1e-15)
    for _ in range(7):
        agent.step(AG.LOOK_DOWN)
    # in the open a forward step moves exactly forward_step along f
    agent.step(AG.TURN_LEFT)
    f = agent.forward
    assert np.allclose(f, [-np.sin(np.radians(10.0)), -np.cos(np.radians(10.0))], atol=1e-16)
    before = np.array([agent.x, agent.z])
    assert agent.step(AG.MOVE_FORWARD)
    after = np.array([agent.x, agent.z])
    assert np.array_equal(after, before + 1.0 * agent.forward_step * f) and abs(np.linalg.norm(after - before) - 0.065) < 1e-15
    assert agent.path_length == 0.065
    # head-on into the wall at z = -1: rows 3 and 4 touch it, row 5 is within the radius; the first cell that is not free is row 5, whose
    # border towards the agent is z = -1.25 + 6 / 16 = -0.875
    agent = AG.SimAgent(nav, (-0.3, 0.0))
    border, moved, hit = -0.875, 0, None
    for i in range(40):
        z = agent.z
        done = agent.step(AG.MOVE_FORWARD)
        assert nav.is_free(agent.x, agent.z) and agent.x == -0.3 and agent.z <= z
        if not done:
            hit = i
            break
    assert hit is not None and border <= agent.z <= border + nav.cell / 4 + nav.cell, (hit, agent.z)
    assert hit == 13                                                             # 0.875 m at 0.065 m a step: the 14th step is cut short
    z = agent.z
    assert agent.z - border < agent.forward_step / agent.substeps + 1e-12        # the sub-step is the resolution
    for _ in range(3):
        assert not agent.step(AG.MOVE_FORWARD) and agent.z == z
    assert agent.path_length == 17 * 0.065                                       # actions are counted, not displacement
    # actions.txt round trip and replay
    path = os.path.join(str(tmp_path), "actions.txt")
    rng = np.random.RandomState(5)
    actions = [int(a) for a in rng.choice([1, 1, 1, 2, 3, 3, 4, 5, 0], 120)]
    a1 = AG.SimAgent(nav, (0.3, -0.2), heading_steps=3)
    results = AG.replay(a1, actions)
    AG.save_actions(path, a1.actions)
    with open(path) as fh:
        assert fh.read() == "".join(f"{a}\n" for a in actions)
    a2 = AG.SimAgent(nav, (0.3, -0.2), heading_steps=3)
    assert AG.replay(a2, AG.load_actions(path)) == results and a2.X_WV.tobytes() == a1.X_WV.tobytes() and a2.actions == actions
    assert a1.path_length == actions.count(1) * 0.065 and not all(results)
    # refusals
    with pytest.raises(ValueError, match="not free"):
        AG.SimAgent(nav, (0.6, 0.3))                                             # inside the pillar
    with pytest.raises(ValueError, match="not free"):
        AG.SimAgent(nav, (9.0, 0.0))                                             # outside the grid
    with pytest.raises(ValueError, match="unknown action"):
        a1.step(6)


def check_agent_follows_sensor_poses(device):
    """tests/mesh_cases.py:sensor_poses -- 0.25 m forward and a 10 degree turn per frame, from (0, 0, 1.5) -- as actions.  sensor_poses adds
    np.deg2rad(10) five times where the agent converts count * 10 degrees once: the yaw differs by at most five roundings of about 1e-16, the
    position by that times the 1.25 m walked.  Bound: 1e-14."""
    v, t, _ = mc.flat_room()
    nav = AG.NavGrid.build(S.MeshScene(v, t, device=device), origin_xz=(-2.0, -3.0), cell=0.125, grid_shape=(48, 32), floor_y=-1.2)
    assert (n(nav.grid)[2:-2, 2:-2] == 1).all() and (n(nav.grid)[0] == 3).all()
    agent = AG.SimAgent(nav, (0.0, 1.5), forward_step=0.25, sensor_height=1.2)
    poses = mc.sensor_poses(6)
    for i, X in enumerate(poses):
        assert np.abs(agent.X_WV - X).max() <= 1e-14, (i, np.abs(agent.X_WV - X).max())
        assert agent.step(AG.MOVE_FORWARD) and agent.step(AG.TURN_LEFT)

# ---- judge, frames, closed loop -------------------------------------------------------------------------------------------------------------

SENSOR_W, SENSOR_H = 64, 48


def sensor_of(scene):
    from activesplat_amd import synthetic as syn
    K = syn.intrinsics(SENSOR_W, SENSOR_H, fx=32.0, fy=32.0)
    return S.MeshSensor(scene, K, SENSOR_W, SENSOR_H), K


def check_judge_actions(device):
    v, t = reference("room")[0]
    scene = S.MeshScene(v, t, device=device)
    nav = AG.NavGrid.build(scene, **GRID, floor_y=FLOOR_Y)
    sensor, _ = sensor_of(scene)
    samples = S.sample_surface(scene, 1500, uniforms=torch.from_numpy(np.random.RandomState(3).uniform(size=(1500, 3))))
    actions = [2, 2, 2, 1, 1, 3, 3, 3, 3, 3, 3, 1, 4, 5, 0]
    agent = AG.SimAgent(nav, (-0.3, 0.0), turn_angle=30.0)
    rows = AG.judge_actions(scene, sensor, agent, actions, samples)
    assert rows.shape == (len(actions) + 1, 6) and agent.actions == actions
    ratio = rows[:, 1]
    print("judge_actions: completion ratio per frame", ratio.tolist())
    assert (np.diff(ratio) >= 0).all() and ratio[-1] > ratio[0] > 0.0
    forwards = np.cumsum([0] + [int(a == 1) for a in actions])
    assert np.array_equal(rows[:, 4], forwards * 0.065)
    with pytest.raises(ValueError, match="scene"):
        AG.judge_actions(S.MeshScene(v, t, device=device), sensor, agent, [], samples)


def check_frames(device):
    """a waypoint given in the mapper's world, carried to the simulator's world, marked there with a small triangle and rendered from a later pose:
    the marker appears at the pixel the mapper-world point projects to through the view matrix `plan_step` is given"""
    v, t = reference("room")[0]
    scene = S.MeshScene(v, t, device=device)
    nav = AG.NavGrid.build(scene, **GRID, floor_y=FLOOR_Y)
    sensor, K = sensor_of(scene)
    agent = AG.SimAgent(nav, (-0.3, 0.1), heading_steps=4)                      # a first pose that is neither at the origin nor axis-aligned
    X0 = agent.X_WV
    for a in (1, 1, 3, 3, 3, 1, 2):
        agent.step(a)
    X = agent.X_WV
    # the first camera sits at the mapper's origin and looks along its +z; the floor is 1.25 m below it, along +y
    assert np.allclose(EX.view_c2w(sensor, X0, X0), np.eye(4), atol=1e-12)
    feet = EX.sim_to_mapper(sensor, X0) @ np.array([X0[0, 3], FLOOR_Y, X0[2, 3], 1.0])
    assert np.allclose(feet, [0.0, 1.25, 0.0, 1.0], atol=1e-12)
    c2w = EX.view_c2w(sensor, X0, X)
    k = np.asarray(K, np.float64)
    for pix in ((20.0, 30.0), (41.0, 12.0)):
        # a point 0.8 m in front of the later camera, on the ray of pixel `pix`, expressed in the mapper's world
        ray = np.array([(pix[0] - k[0, 2]) / k[0, 0], (pix[1] - k[1, 2]) / k[1, 1], 1.0]) * 0.8
        p_mapper = c2w[:3, :3] @ ray + c2w[:3, 3]
        p_sim = EX.points_to_sim(sensor, X0, p_mapper[None])[0]
        assert np.allclose(EX.sim_to_mapper(sensor, X0) @ np.append(p_sim, 1.0), np.append(p_mapper, 1.0), atol=1e-12)
        # the marker: a triangle of 4 cm around the point, facing the camera
        right, up = X[:3, 0], X[:3, 1]
        mv = np.stack([p_sim - 0.02 * right - 0.02 * up, p_sim + 0.02 * right - 0.02 * up, p_sim + 0.02 * up]).astype(np.float32)
        marker = S.MeshScene(mv, np.array([[0, 1, 2]], np.int32), device=device)
        _, depth, tri_id = S.render_mesh(marker, sensor.k4, sensor.w2c(X), SENSOR_W, SENSOR_H)
        hit = n(tri_id) >= 0
        assert hit.any() and hit[int(pix[1]), int(pix[0])], (pix, np.argwhere(hit).tolist())
        rows, cols = np.nonzero(hit)
        assert abs(rows.mean() - pix[1]) <= 1.0 and abs(cols.mean() - pix[0]) <= 1.0
        assert abs(float(n(depth)[int(pix[1]), int(pix[0])]) - 0.8) < 1e-3
    assert np.allclose(EX.quat_wxyz(np.diag([-1.0, 1.0, -1.0])), [0.0, 0.0, 1.0, 0.0]) and np.allclose(EX.quat_wxyz(np.eye(3)), [1.0, 0.0, 0.0, 0.0])
    for X_ in (X0, X):
        q = EX.quat_wxyz(X_[:3, :3]).astype(np.float64)
        assert np.allclose(q, mc._quat(X_[:3, :3]), atol=1e-6) or np.allclose(-q, mc._quat(X_[:3, :3]), atol=1e-6)


# the planner's window in the MAPPER'S world of an agent that starts level with yaw 0 at the simulator's (start_x, ., start_z): mapper x = x -
# start_x, mapper z = -(z - start_z), mapper y = -(y - sensor height); the band keeps what lies between 0.1 m above the floor and the head
def plan_window(start_xz, x_range, z_range, px_per_m=16):
    cx, cz = 0.5 * (x_range[0] + x_range[1]) - start_xz[0], -(0.5 * (z_range[0] + z_range[1]) - start_xz[1])
    sx, sz = x_range[1] - x_range[0], z_range[1] - z_range[0]
    return dict(world_center=(cx, cz), world_shape=(sx, sz), grid_shape=(int(sx * px_per_m), int(sz * px_per_m)), upper=-1.15, lower=0.25,
                agent_radius=0.1, node_spacing=0.5, scale_modifier=1.0)


def explorer_of(device, mesh, grid, start_xz, window, frames, turn_angle, judge, policy=True, bootstrap_turns=None, look_down_steps=1):
    from activesplat_amd import judge as J
    from activesplat_amd import policy as PL
    from activesplat_amd.mapper import SplatMapper
    scene = S.MeshScene(*mesh, device=device)
    nav = AG.NavGrid.build(scene, floor_y=FLOOR_Y, **grid)
    sensor, K = sensor_of(scene)
    agent = AG.SimAgent(nav, start_xz, turn_angle=turn_angle, tilt_angle=45.0)
    mp = SplatMapper(K, SENSOR_W, SENSOR_H, config=dict(step_num=frames, densify_downscale_factor=2, device_ingest=True), device=device)
    if judge:
        samples = S.sample_surface(scene.transformed(sensor.w2c(agent.X_WV)), 2000, uniforms=torch.from_numpy(np.random.RandomState(3).uniform(size=(2000, 3))))
        mp.judge = J.CompletionJudge(samples)
    px_per_m = window["grid_shape"][0] / window["world_shape"][0]
    pol = PL.SubregionPolicy(step_px=agent.forward_step * px_per_m, radius_px=window["agent_radius"] * px_per_m) if policy else None
    return EX.Explorer(mp, sensor, agent, window, policy=pol, bootstrap_turns=bootstrap_turns, look_down_steps=look_down_steps), nav


def check_episode(out, nav, budget):
    assert 0 < len(out["actions"]) <= budget and all(a in AG.ACTIONS for a in out["actions"])
    assert out["positions"].shape == (len(out["actions"]) + 1, 2) and len(out["completed"]) == len(out["actions"])
    assert all(nav.is_free(x, z) for x, z in out["positions"]), "every position is free"
    assert out["plans"] >= 1 and len(out["nodes"]) == out["plans"]
    assert out["collisions"] == sum(1 for a, done in zip(out["actions"], out["completed"]) if a == AG.MOVE_FORWARD and not done)


def check_closed_loop_short(device):
    """a shortened episode in the dyadic room: 30 degree turns, a 64 x 48 sensor, a handful of actions after the bootstrap.  The bootstrap
    looks down once (45 degrees) for a second circle: without it the floor under the agent is never seen and no plan finds a node."""
    mesh = reference("room")[0]
    v, t = mesh
    colours = np.random.RandomState(7).randint(40, 256, (len(v), 3)).astype(np.uint8)
    budget = (12 + 1 + 12 + 1) + 6                # the bootstrap (a circle, a look down, a circle, a look up) and six actions
    ex, nav = explorer_of(device, (v, t, colours), GRID, (-0.3, 0.0), plan_window((-0.3, 0.0), (-1.5, 1.5), (-1.25, 1.25)), budget + 2, 30.0, judge=False)
    out = ex.run(budget)
    print("short episode:", out["actions"], "plans", out["plans"], "nodes", out["nodes"], "arrivals", out["arrivals"], "collisions", out["collisions"])
    check_episode(out, nav, budget)
    assert ex.bootstrap_actions == 26 and out["actions"][:26] == [AG.TURN_LEFT] * 12 + [AG.LOOK_DOWN] + [AG.TURN_LEFT] * 12 + [AG.LOOK_UP]
    assert out["judge"] is None and out["nodes"][0] >= 0, "the first plan finds a node"
    if out["nodes"][-1] >= 0:
        assert len(out["actions"]) == budget, "the loop ends only when there is no node or the budget is spent"


TWO_ROOMS_GRID = dict(origin_xz=(-1.5, -1.0), cell=0.0625, grid_shape=(32, 48))
TWO_ROOMS_START = (-0.625, 0.0)
TWO_ROOMS_BUDGET = 2 * 38           # twice the number of actions at which the completion ratio first exceeded the bootstrap's (profiles/agent.txt)


def two_rooms_explorer(device, budget):
    window = plan_window(TWO_ROOMS_START, (-1.5, 1.5), (-1.0, 1.0))
    return explorer_of(device, two_rooms(), TWO_ROOMS_GRID, TWO_ROOMS_START, window, budget + 2, 30.0, judge=True)


def check_closed_loop_two_rooms(device, budget=TWO_ROOMS_BUDGET):
    """GPU only.  Two dyadic rooms joined by a door; the mapper configuration of tests/mesh_cases.py:run_sequence with `mapper.judge` set."""
    ex, nav = two_rooms_explorer(device, budget)
    out = ex.run(budget)
    ratio = out["judge"][:, 1]
    after_bootstrap = ratio[ex.bootstrap_actions]
    first = int(np.argmax(ratio > after_bootstrap)) if (ratio > after_bootstrap).any() else -1
    print(f"two rooms: {len(out['actions'])} actions, plans {out['plans']} nodes {out['nodes']} arrivals {out['arrivals']} collisions {out['collisions']}; "
          f"completion ratio {ratio[0]:.4f} at the start, {after_bootstrap:.4f} after the bootstrap, {ratio[-1]:.4f} at the end; first above the "
          f"bootstrap's at frame {first}")
    check_episode(out, nav, budget)
    assert out["judge"].shape == (len(out["actions"]) + 1, 6)
    assert any(node >= 0 for node in out["nodes"]), "at least one plan found a node"
    assert out["arrivals"] >= 1
    assert ratio[-1] > after_bootstrap, (ratio[-1], after_bootstrap)
    return out
