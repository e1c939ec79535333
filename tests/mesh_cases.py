"""Shared checks of the mesh RGB-D sensor (activesplat_amd/sensor.py; gs_mesh_render): run on the host-emulated kernels by
tests/test_mesh_sensor.py and on the MI355X by tests/test_gpu_mesh_sensor.py.

Expected values
* `restate(...)`: the rendering rule of include/gsplat_hip.h (gs_mesh_render) written in numpy, brute force over all triangles, in float64 (the
  expected image) and in float32 (only to measure how far a float32 evaluation of the same rule lies from the float64 one: the depth tolerance
  of a case is 8 x that worst relative error, floor 1e-6 -- the factor allows for fused multiply-adds and another summation order in the kernel).
  Nothing from the code under test goes into them.
* Edge-critical pixels.  The float64 restatement flags a pixel when
    (a) some triangle has its smallest barycentric weight min(U/S, V/S, W/S) within +-1e-4 of zero, passes the near test within the same relative
        margin (z >= near (1 - 1e-4)) and is no farther than the winner by 1e-4 relative (z <= z_winner (1 + 1e-4); any z when nothing is hit), or
    (b) the two nearest hits are within 1e-4 relative of each other.
  On flagged pixels only "hit or not" is compared; on every other pixel tri_id must be equal, depth within the tolerance, colour within one
  level.  The share of flagged pixels is capped per case (1 % at generic poses, 5 % at the axis-aligned pose, where quad diagonals run through
  pixel centres); the cap is asserted on the reference alone, before anything is compared.
* `restate_samples`: sample_surface's rule in numpy float64.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from activesplat_amd import _lib
from activesplat_amd import rasterizer as R
from activesplat_amd import sensor as S

GS_EINVAL = 1
MARGIN = 1e-4
ROOM = ((-2.0, 2.0), (-1.2, 1.2), (-3.0, 3.0))

# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------------


def restate(vertices, triangles, colors, k4, w2c, W, H, near, dtype=np.float64, chunk=96):
    """gs_mesh_render's rule in `dtype`, every triangle against every pixel -> dict(depth [H,W], tri_id [H,W], color [H,W,3] uint8, and for
    float64 also flagged [H,W] bool)"""
    f = dtype
    v = np.asarray(vertices, np.float32).astype(f)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).astype(f)
    m = np.asarray(w2c, np.float64)[:3].astype(np.float32).astype(f)
    fx, fy, cx, cy = (f(np.float32(a)) for a in k4)
    near_f = f(np.float32(near))
    p = np.stack([m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1] + m[r, 2] * v[:, 2] + m[r, 3] for r in range(3)], 1)
    dx = ((np.arange(W).astype(f) - cx) / fx)[None, None, :]
    dy = ((np.arange(H).astype(f) - cy) / fy)[None, :, None]
    inf = f(np.inf)
    best_z, second_z = np.full((H, W), inf, f), np.full((H, W), inf, f)
    best_id = np.full((H, W), -1, np.int64)
    best_uvw = np.zeros((3, H, W), f)
    edge_z = np.full((H, W), inf, np.float64)             # nearest triangle that is within the margin of one of its edges (condition a)

    def edge(i, j):
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        a, b = p[lo], p[hi]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        e = dx * n[:, 0, None, None] + dy * n[:, 1, None, None] + n[:, 2, None, None]
        return np.where((i > j)[:, None, None], -e, e)

    with np.errstate(all="ignore"):
        for c0 in range(0, len(tri), chunk):
            t = tri[c0:c0 + chunk]
            a, b, c = t[:, 0], t[:, 1], t[:, 2]
            U, V, Wt = edge(b, c), edge(c, a), edge(a, b)
            Ssum = U + V + Wt
            za, zb, zc = (p[i, 2][:, None, None] for i in (a, b, c))
            z = (U * za + V * zb + Wt * zc) / Ssum
            same = ((U >= 0) & (V >= 0) & (Wt >= 0)) | ((U <= 0) & (V <= 0) & (Wt <= 0))
            hit = same & (Ssum != 0) & np.isfinite(z) & (z >= near_f)
            zs = np.where(hit, z, inf)
            k = np.argmin(zs, 0)                           # (the first of equal minima: the lowest index of the chunk)
            zk = np.take_along_axis(zs, k[None], 0)[0]
            # the second nearest of (what was known, this chunk)
            rest = zs.copy()
            np.put_along_axis(rest, k[None], inf, 0)
            z2 = rest.min(0)
            better = zk < best_z                           # strict: an equal z of a later chunk has the higher index
            second_z = np.where(better, np.minimum(best_z, z2), np.minimum(second_z, np.minimum(zk, z2)))
            for q, E in enumerate((U, V, Wt)):
                best_uvw[q] = np.where(better, np.take_along_axis(E, k[None], 0)[0], best_uvw[q])
            best_id = np.where(better, c0 + k, best_id)
            best_z = np.where(better, zk, best_z)
            if f is np.float64:
                wmin = np.minimum(np.minimum(U / Ssum, V / Ssum), Wt / Ssum)
                crit = (np.abs(wmin) <= MARGIN) & np.isfinite(z) & (z >= near_f * (1 - MARGIN))
                edge_z = np.minimum(edge_z, np.where(crit, z, np.inf).min(0))
        hit = best_id >= 0
        Ssum = best_uvw[0] + best_uvw[1] + best_uvw[2]
        safe = np.where(hit, best_id, 0)
        color = np.zeros((H, W, 3), np.uint8)
        for ch in range(3):
            ca, cb, cc = (col[tri[safe, q], ch] for q in range(3))
            level = np.floor((best_uvw[0] * ca + best_uvw[1] * cb + best_uvw[2] * cc) / Ssum + f(0.5))
            color[..., ch] = np.where(hit, np.clip(level, 0, 255), 0).astype(np.uint8)
        out = dict(depth=np.where(hit, best_z, 0).astype(f), tri_id=np.where(hit, best_id, -1).astype(np.int32), color=color)
        if f is np.float64:
            out["flagged"] = (np.isfinite(edge_z) & (edge_z <= best_z * (1 + MARGIN))) | (hit & (second_z <= best_z * (1 + MARGIN)))
    return out


def restate_samples(vertices, triangles, u):
    """sample_surface's rule in numpy float64 -> (points float32 [n,3], face [n])"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    tri = np.asarray(triangles, np.int64)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    cum = np.cumsum(area)
    face = np.minimum(np.searchsorted(cum, u[:, 0] * cum[-1], side="right"), len(tri) - 1)
    r1, r2 = u[:, 1].copy(), u[:, 2].copy()
    fold = r1 + r2 > 1.0
    r1[fold], r2[fold] = 1.0 - r1[fold], 1.0 - r2[fold]
    pts = a[face] + r1[:, None] * (b[face] - a[face]) + r2[:, None] * (c[face] - a[face])
    return pts.astype(np.float32), face

# ---- scenes and poses -----------------------------------------------------------------------------------------------------------------------


def box(lo_hi):
    (x0, x1), (y0, y1), (z0, z1) = lo_hi
    v = np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)], np.float32)
    quads = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))
    t = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int32)
    return v, t


def merge(parts):
    vs, ts, n = [], [], 0
    for v, t in parts:
        vs.append(v); ts.append(t + n); n += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts).astype(np.int32)


def random_scene(seed=0):
    """the room box, a furniture box and 150 random triangles, random vertex colours"""
    rng = np.random.RandomState(seed)
    centres = np.stack([rng.uniform(lo, hi, 150) for lo, hi in ROOM], 1)
    rv = (centres[:, None, :] + rng.normal(0.0, 0.25, (150, 3, 3))).reshape(-1, 3).astype(np.float32)
    v, t = merge([box(ROOM), box(((0.4, 1.1), (-1.2, -0.3), (0.8, 1.6))), (rv, np.arange(450, dtype=np.int32).reshape(150, 3))])
    return v, t, rng.randint(0, 256, (len(v), 3)).astype(np.uint8)


def flat_room():
    v, t = box(ROOM)
    rng = np.random.RandomState(4)
    return v, t, rng.randint(40, 256, (len(v), 3)).astype(np.uint8)


def bumpy_room(n=12, seed=1):
    """six walls of n x n quads on the room box; the lattice vertices are shared between quads and walls and jittered by N(0, 0.01^2)"""
    rng = np.random.RandomState(seed)
    index, verts = {}, []

    def vid(i, j, k):
        if (i, j, k) not in index:
            index[(i, j, k)] = len(verts)
            verts.append([ROOM[0][0] + (ROOM[0][1] - ROOM[0][0]) * i / n, ROOM[1][0] + (ROOM[1][1] - ROOM[1][0]) * j / n,
                          ROOM[2][0] + (ROOM[2][1] - ROOM[2][0]) * k / n])
        return index[(i, j, k)]
    tris = []
    for axis in range(3):
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def at(da, db):
                        ijk = [0, 0, 0]
                        ijk[axis] = side
                        ijk[(axis + 1) % 3], ijk[(axis + 2) % 3] = a + da, b + db
                        return vid(*ijk)
                    q = (at(0, 0), at(1, 0), at(1, 1), at(0, 1))
                    tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    v = (np.array(verts) + rng.normal(0.0, 0.01, (len(verts), 3))).astype(np.float32)
    return v, np.array(tris, np.int32), rng.randint(0, 256, (len(v), 3)).astype(np.uint8)


def crossing_scene():
    """a floor of two large triangles passing under and behind the camera (y is down), a wall triangle with one vertex behind the camera, a
    triangle wholly behind it"""
    v = np.array([[-20, 1.0, -20], [20, 1.0, -20], [20, 1.0, 20], [-20, 1.0, 20],
                  [-1.5, -1.0, 3.0], [1.2, 0.9, 2.5], [0.4, -0.3, -1.0],
                  [-1.0, -1.0, -2.0], [1.0, -1.0, -2.0], [0.0, 1.0, -3.0]], np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9]], np.int32)
    c = np.array([[200, 30, 30]] * 4 + [[30, 200, 30]] * 3 + [[30, 30, 200]] * 3, np.uint8)
    return v, t, c


def pose(yaw, pitch, roll, position):
    """world-to-camera 4x4 of a camera at `position` with c2w rotation Ry(yaw) Rx(pitch) Rz(roll) (x right, y down, z forward)"""
    cy_, sy = np.cos(yaw), np.sin(yaw)
    cp, sp = np.cos(pitch), np.sin(pitch)
    cr, sr = np.cos(roll), np.sin(roll)
    ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    c2w = np.eye(4)
    c2w[:3, :3] = ry @ rx @ rz
    c2w[:3, 3] = position
    return np.linalg.inv(c2w)


def k_for(W, H, f):
    return np.array([f, f, W / 2 - 1, H / 2 - 1], np.float32)


GENERIC_POSES = (pose(0.47, -0.14, 0.05, (0.3, 0.1, -0.4)), pose(2.1, 0.2, -0.1, (-0.7, -0.3, 1.0)), pose(4.0, -0.35, 0.0, (1.2, 0.4, -2.0)))
AXIS_POSE = np.eye(4)
NEAR = 0.05

# ---- comparison -----------------------------------------------------------------------------------------------------------------------------

_reference = {}


def reference(key, mesh, k4, w2c, W, H, near, everywhere=False):
    """(float64 restatement, depth tolerance) of a case, computed once per session and shared"""
    if key not in _reference:
        v, t, c = mesh
        r64 = restate(v, t, c, k4, w2c, W, H, near, np.float64)
        r32 = restate(v, t, c, k4, w2c, W, H, near, np.float32)
        both = (r64["tri_id"] >= 0) & (r32["tri_id"] >= 0)
        if not everywhere:
            both &= ~r64["flagged"] & (r64["tri_id"] == r32["tri_id"])
        rel = np.abs(r32["depth"].astype(np.float64) - r64["depth"])[both] / r64["depth"][both]
        r64["fp32_rel"] = float(rel.max()) if rel.size else 0.0
        r64["fp32_id_diff"] = int((r64["tri_id"] != r32["tri_id"]).sum())
        r64["fp32_id_diff_unflagged"] = int(((r64["tri_id"] != r32["tri_id"]) & ~r64["flagged"]).sum())
        for a in r64.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _reference[key] = (r64, max(1e-6, 8.0 * r64["fp32_rel"]))
    return _reference[key]


def render(device, mesh, k4, w2c, W, H, near, scene=None):
    scene = scene if scene is not None else S.MeshScene(*mesh, device=device)
    color, depth, tri_id = S.render_mesh(scene, k4, w2c, W, H, near)
    assert color.shape == (H, W, 3) and color.dtype == torch.uint8 and depth.shape == (H, W) and depth.dtype == torch.float32
    assert tri_id.shape == (H, W) and tri_id.dtype == torch.int32
    return color.cpu().numpy(), depth.cpu().numpy(), tri_id.cpu().numpy()


def compare(what, got, ref, tol, cap, everywhere=False):
    """the comparison rule of this file's docstring; everywhere: the depth of EVERY pixel within tol (a closed surface)"""
    color, depth, tri_id = got
    flagged = ref["flagged"]
    share = float(flagged.mean())
    assert share <= cap, (what, "flagged share", share)
    hit = ref["tri_id"] >= 0
    rel = np.abs(depth.astype(np.float64) - ref["depth"]) / np.where(hit, ref["depth"], 1.0)
    ok = ~flagged
    print(f"{what}: flagged {100 * share:.3f} %  numpy-fp32 worst rel {ref['fp32_rel']:.2e} (ids differing {ref['fp32_id_diff']}, unflagged "
          f"{ref['fp32_id_diff_unflagged']})  tolerance {tol:.2e}  kernel worst rel: unflagged {rel[ok & hit].max() if (ok & hit).any() else 0.0:.2e} "
          f"all {rel[hit].max() if hit.any() else 0.0:.2e}  ids differing: {int((tri_id != ref['tri_id']).sum())} (unflagged {int(((tri_id != ref['tri_id']) & ok).sum())})")
    assert np.array_equal(tri_id >= 0, hit), (what, "hit mask", int(((tri_id >= 0) != hit).sum()))
    assert np.array_equal(depth == 0, ~hit) and np.array_equal(color[~hit], np.zeros_like(color[~hit])), (what, "cleared where nothing is hit")
    assert np.array_equal(tri_id[ok], ref["tri_id"][ok]), (what, "tri_id", int((tri_id[ok] != ref["tri_id"][ok]).sum()))
    where = hit if everywhere else (ok & hit)
    assert (rel[where] <= tol).all(), (what, "depth", float(rel[where].max()), tol)
    assert np.abs(color[ok].astype(np.int32) - ref["color"][ok].astype(np.int32)).max(initial=0) <= 1, (what, "colour")

# ---- the checks -----------------------------------------------------------------------------------------------------------------------------


def check_random_scene(device):
    mesh = random_scene()
    scene = S.MeshScene(*mesh, device=device)
    W, H = 48, 40
    k4 = k_for(W, H, 24.0)
    for i, w2c in enumerate(GENERIC_POSES + (AXIS_POSE,)):
        ref, tol = reference(("random", i), mesh, k4, w2c, W, H, NEAR)
        compare(f"random scene pose {i}", render(device, mesh, k4, w2c, W, H, NEAR, scene), ref, tol, 0.05 if i == 3 else 0.01)


def check_partial_tiles(device):
    mesh = random_scene()
    for W, H in ((37, 21), (16, 16)):
        k4 = k_for(W, H, 24.0)
        ref, tol = reference(("partial", W, H), mesh, k4, GENERIC_POSES[0], W, H, NEAR)
        compare(f"partial tiles {W} x {H}", render(device, mesh, k4, GENERIC_POSES[0], W, H, NEAR), ref, tol, 0.01)


BUMPY_POSES = (pose(0.47, -0.14, 0.05, (0.3, 0.1, -0.4)), pose(2.1, 0.2, -0.1, (-0.7, -0.3, 1.0)), pose(0.6, -0.3, 0.1, (1.7, -0.9, 2.7)))


def check_closed_room(device):
    """watertightness: every pixel of a closed room is hit, and -- the surface being continuous -- every depth is within the tolerance"""
    mesh = bumpy_room()
    assert len(mesh[1]) == 1728
    scene = S.MeshScene(*mesh, device=device)
    W, H = 96, 80
    k4 = k_for(W, H, 48.0)
    for i, w2c in enumerate(BUMPY_POSES):
        ref, tol = reference(("bumpy", i), mesh, k4, w2c, W, H, NEAR, everywhere=True)
        assert (ref["tri_id"] >= 0).all()
        got = render(device, mesh, k4, w2c, W, H, NEAR, scene)
        assert (got[2] >= 0).all(), (i, "holes", int((got[2] < 0).sum()))
        compare(f"closed bumpy room pose {i}", got, ref, tol, 0.01, everywhere=True)


def check_near_plane(device):
    mesh = crossing_scene()
    W, H = 48, 40
    k4 = k_for(W, H, 24.0)
    for i, w2c in enumerate((pose(0.11, 0.07, 0.03, (0.0, 0.0, 0.0)), pose(0.4, 0.45, -0.2, (0.3, -0.2, 0.1)))):
        ref, tol = reference(("crossing", i), mesh, k4, w2c, W, H, NEAR)
        seen = set(np.unique(ref["tri_id"]).tolist())
        assert {0, 1}.issubset(seen) and 3 not in seen and (i == 1 or 2 in seen), seen     # the floor is seen, the triangle behind is not
        compare(f"near-plane crossing pose {i}", render(device, mesh, k4, w2c, W, H, NEAR), ref, tol, 0.01)


def check_known_answers(device):
    W, H = 48, 40
    k4 = k_for(W, H, 24.0)
    # one triangle at z = 2 facing the camera: exactly 2 inside, the covered pixels are the restatement's
    v = np.array([[-1.03, -0.97, 2.0], [1.11, -0.83, 2.0], [0.07, 1.09, 2.0]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    c = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    ref = restate(v, t, c, k4, np.eye(4), W, H, NEAR)
    color, depth, tri_id = render(device, (v, t, c), k4, np.eye(4), W, H, NEAR)
    assert np.array_equal(tri_id >= 0, ref["tri_id"] >= 0) and 100 < int((tri_id >= 0).sum()) < W * H
    assert np.array_equal(depth, np.where(tri_id >= 0, np.float32(2.0), np.float32(0.0)))
    ok = ~ref["flagged"]
    assert np.abs(color[ok].astype(np.int32) - ref["color"][ok].astype(np.int32)).max() <= 1
    # the same triangle listed twice: the lower index wins everywhere
    _, depth2, tri_id2 = render(device, (v, np.array([[0, 1, 2], [0, 1, 2]], np.int32), c), k4, np.eye(4), W, H, NEAR)
    assert np.array_equal(tri_id2, np.where(tri_id >= 0, 0, -1)) and np.array_equal(depth2, depth)
    # a uniform-colour mesh gives exactly that colour on every hit pixel
    rv, rt, _ = random_scene()
    uniform = np.tile(np.array([[37, 180, 92]], np.uint8), (len(rv), 1))
    color, _, tri_id = render(device, (rv, rt, uniform), k4, GENERIC_POSES[0], W, H, NEAR)
    assert (tri_id >= 0).all() and np.array_equal(color, np.broadcast_to(np.array([37, 180, 92], np.uint8), color.shape))
    # the default colour is mid-grey
    color, _, _ = render(device, (rv, rt, None), k4, GENERIC_POSES[0], W, H, NEAR)
    assert np.array_equal(color, np.full_like(color, 128))
    # a degenerate triangle and an empty scene give cleared outputs
    for tris in (np.array([[0, 0, 1], [2, 1, 1]], np.int32), np.zeros((0, 3), np.int32)):
        color, depth, tri_id = render(device, (v, tris, c), k4, np.eye(4), W, H, NEAR)
        assert (tri_id == -1).all() and (depth == 0).all() and (color == 0).all()
    color, depth, tri_id = render(device, (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None), k4, np.eye(4), 5, 3, NEAR)
    assert (tri_id == -1).all() and (depth == 0).all() and (color == 0).all()


def _abi_call(device, scene, k4, w2c, W, H, near, capacity, guard=4096, **over):
    """gs_mesh_render with a scratch of exactly the layout's size followed by guard bytes -> (rc, outputs, counts, guard intact)"""
    lib = _lib.get()
    T = scene.num_triangles
    layout = _lib.GsMeshLayout()
    assert lib.gs_mesh_render_layout(T, W, H, capacity, C.byref(layout)) == 0
    n = int(layout.total_bytes)
    buf = torch.full((n + guard,), 0xAB, dtype=torch.uint8, device=device)
    depth = torch.full((H, W), -7.0, dtype=torch.float32, device=device)
    tri_id = torch.full((H, W), -7, dtype=torch.int32, device=device)
    color = torch.full((H, W, 3), 7, dtype=torch.uint8, device=device)
    counts = torch.zeros(2, dtype=torch.int32, device=device)
    k = np.asarray(k4, np.float32).copy()
    m = np.ascontiguousarray(np.asarray(w2c, np.float64)[:3].reshape(12), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    a = dict(num_vertices=scene.num_vertices, vertices=R._ptr(scene.vertices), num_triangles=T, triangles=R._ptr(scene.triangles),
             colors=R._ptr(scene.vertex_colors), k=k.ctypes.data_as(fp), m=m.ctypes.data_as(fp), near_z=float(near), width=W, height=H, scratch=R._ptr(buf),
             capacity=capacity, depth=R._ptr(depth), tri_id=R._ptr(tri_id), color=R._ptr(color), counts=R._ptr(counts))
    a.update(over)
    rc = lib.gs_mesh_render(a["num_vertices"], a["vertices"], a["num_triangles"], a["triangles"], a["colors"], a["k"], a["m"], a["near_z"], a["width"], a["height"],
                            a["scratch"], a["capacity"], a["depth"], a["tri_id"], a["color"], a["counts"], _lib.stream_ptr(torch.device(device)))
    return rc, (color.cpu().numpy(), depth.cpu().numpy(), tri_id.cpu().numpy()), [int(x) & 0xffffffff for x in counts.tolist()], \
        bool((buf[n:] == 0xAB).all()), layout


def check_capacity(device):
    mesh = random_scene()
    scene = S.MeshScene(*mesh, device=device)
    W, H = 48, 40
    k4, w2c = k_for(W, H, 24.0), GENERIC_POSES[0]
    ref, tol = reference(("random", 0), mesh, k4, w2c, W, H, NEAR)
    rc, (color, depth, tri_id), (need, longest), intact, layout = _abi_call(device, scene, k4, w2c, W, H, NEAR, capacity=1)
    tiles = 3 * 3
    assert rc == 0 and intact and need > tiles and need >= longest >= (need + tiles - 1) // tiles
    assert int(layout.total_bytes) >= int(layout.list) + 4
    assert (tri_id == -1).all() and (depth == 0).all() and (color == 0).all()                 # an overflowed launch leaves no image
    rc, got, (need2, longest2), intact, _ = _abi_call(device, scene, k4, w2c, W, H, NEAR, capacity=need)
    assert rc == 0 and intact and (need2, longest2) == (need, longest)
    compare("capacity = D", got, ref, tol, 0.01)
    # render_mesh starting from capacity 1 returns the right image and remembers what was needed
    scene.capacities[(W, H)] = 1
    compare("render_mesh from capacity 1", render(device, mesh, k4, w2c, W, H, NEAR, scene), ref, tol, 0.01)
    assert scene.capacities[(W, H)] >= need and scene.last_counts == (need, longest)


def check_repeatable(device):
    mesh = random_scene()
    v, t, c = mesh
    W, H = 48, 40
    k4, w2c = k_for(W, H, 24.0), GENERIC_POSES[1]
    a = render(device, mesh, k4, w2c, W, H, NEAR)
    b = render(device, mesh, k4, w2c, W, H, NEAR)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # another triangle order: the same depth image bit for bit, the same triangles once the ids are mapped back
    perm = np.random.RandomState(9).permutation(len(t))
    color, depth, tri_id = render(device, (v, t[perm], c), k4, w2c, W, H, NEAR)
    assert np.array_equal(depth.view(np.int32), a[1].view(np.int32))
    ref, _ = reference(("random", 1), mesh, k4, w2c, W, H, NEAR)
    ok = ~ref["flagged"]
    mapped = np.where(tri_id >= 0, perm[np.maximum(tri_id, 0)], -1)
    assert np.array_equal(mapped[ok], a[2][ok]) and np.array_equal(color[ok], a[0][ok])


def check_refusals(device):
    lib = _lib.get()
    scene = S.MeshScene(*flat_room(), device=device)
    W, H = 20, 12
    k4, w2c = k_for(W, H, 10.0), np.eye(4)

    def call(**over):
        rc, outs, _, _, _ = _abi_call(device, scene, k4, w2c, W, H, NEAR, 256, **over)
        return rc, outs
    rc, outs = call()
    assert rc == 0 and (outs[2] >= 0).all()                                                   # (the call itself is well formed)
    untouched = lambda outs: (outs[1] == -7).all() and (outs[2] == -7).all() and (outs[0] == 7).all()  # noqa: E731
    for over, text in ((dict(vertices=None), b"null"), (dict(triangles=None), b"null"), (dict(colors=None), b"null"), (dict(scratch=None), b"null"),
                       (dict(depth=None), b"null"), (dict(tri_id=None), b"null"), (dict(color=None), b"null"), (dict(counts=None), b"null"), (dict(k=None), b"null"), (dict(m=None), b"null"),
                       (dict(width=0), b"image size"), (dict(height=16385), b"image size"), (dict(width=16385), b"image size"), (dict(height=0), b"image size"),
                       (dict(num_triangles=-1), b"num_triangles"), (dict(near_z=0.0), b"near"), (dict(near_z=-1.0), b"near"),
                       (dict(near_z=float("inf")), b"near"), (dict(near_z=float("nan")), b"near")):
        rc, outs = call(**over)
        assert rc == GS_EINVAL and text in lib.gs_last_error(), (over, lib.gs_last_error())
        assert untouched(outs), over                                                          # nothing was launched
    fp = C.POINTER(C.c_float)
    for i, bad in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (0, 0.0)):
        k = np.asarray(k4, np.float32).copy()
        k[i] = bad
        rc, outs = call(k=k.ctypes.data_as(fp))
        assert rc == GS_EINVAL and (b"intrinsics" in lib.gs_last_error() or b"fx and fy" in lib.gs_last_error()) and untouched(outs), (i, bad)
    layout = _lib.GsMeshLayout()
    assert lib.gs_mesh_render_layout(-1, W, H, 1, C.byref(layout)) == GS_EINVAL and lib.gs_mesh_render_layout(1, 0, H, 1, C.byref(layout)) == GS_EINVAL
    assert lib.gs_mesh_render_layout(1, W, H, 1, None) == GS_EINVAL
    # the binding's own checks
    v, t, c = flat_room()
    with pytest.raises(ValueError, match="index outside"):
        S.MeshScene(v, np.array([[0, 1, 8]], np.int32), device=device)
    with pytest.raises(ValueError, match="index outside"):
        S.MeshScene(v, np.array([[0, -1, 2]], np.int32), device=device)
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        S.MeshScene(v[:, :2], t, device=device)
    with pytest.raises(ValueError, match=r"\[T, 3\]"):
        S.MeshScene(v, t.reshape(-1), device=device)
    with pytest.raises(TypeError, match="integer"):
        S.MeshScene(v, t.astype(np.float32), device=device)
    with pytest.raises(TypeError, match="floating"):
        S.MeshScene(v.astype(np.int32), t, device=device)
    with pytest.raises(TypeError, match="uint8"):
        S.MeshScene(v, t, c.astype(np.float32), device=device)
    with pytest.raises(ValueError, match="vertex_colors"):
        S.MeshScene(v, t, c[:-1], device=device)
    with pytest.raises(ValueError, match="out of range"):
        S.render_mesh(scene, k4, w2c, 0, 4)
    with pytest.raises(Exception, match="near"):
        S.render_mesh(scene, k4, w2c, 8, 4, near=0.0)
    with pytest.raises(ValueError, match="w2c"):
        S.render_mesh(scene, k4, np.eye(3), 8, 4)
    if torch.device(device).type == "cuda":                  # the product path (the emulated build is the one thing that takes host tensors)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.MeshScene(v, t, c, device="cpu")


def check_sample_surface(device):
    v, t, c = random_scene()
    scene = S.MeshScene(v, t, c, device=device)
    u = np.random.RandomState(11).uniform(size=(3000, 3))
    u[0], u[1], u[2] = (0.0, 0.0, 0.0), (1.0 - 2.0 ** -53, 0.25, 0.25), (0.5, 0.9, 0.9)      # the first face, the last, a folded pair
    got, got_face = S.sample_surface(scene, len(u), uniforms=torch.from_numpy(u), return_faces=True)
    assert got.shape == (len(u), 3) and got.dtype == torch.float32 and got.device.type == torch.device(device).type
    want, face = restate_samples(v, t, u)
    # the same float64 operations in the same association, rounded to float32 once: equal, points and faces
    assert np.array_equal(got_face.cpu().numpy(), face), int((got_face.cpu().numpy() != face).sum())
    assert face[0] == 0 and face[1] == len(t) - 1
    diff = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print("sample_surface: largest difference from the numpy restatement", diff.max())
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, S.sample_surface(scene, len(u), uniforms=torch.from_numpy(u)))   # reproducible to the bit
    # every sample lies in its triangle's plane and inside it (float64; the float32 rounding of the point moves it by less than 5e-7)
    p = got.cpu().numpy().astype(np.float64)
    a, b, cc = (v[t[face, q]].astype(np.float64) for q in range(3))
    n = np.cross(b - a, cc - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(np.einsum("ij,ij->i", p - a, n)).max() <= 1e-6
    m = np.stack([b - a, cc - a], 2)                                                        # [n, 3, 2]
    w12 = np.stack([np.linalg.lstsq(m[i], (p - a)[i], rcond=None)[0] for i in range(len(p))])
    w = np.stack([1.0 - w12.sum(1), w12[:, 0], w12[:, 1]], 1)                               # the weights of a, b, c
    # a negative weight times the height over the opposite edge is how far outside the point lies
    twice_area = np.linalg.norm(np.cross(b - a, cc - a), axis=1)
    height = twice_area[:, None] / np.stack([np.linalg.norm(cc - b, axis=1), np.linalg.norm(a - cc, axis=1), np.linalg.norm(b - a, axis=1)], 1)
    assert (w * height >= -1e-6).all(), float((w * height).min())
    # face counts on areas 1 : 2 : 5 (three triangles in three planes, so the face of a sample is its z)
    tv = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 1], [0, 2, 1], [0, 0, 2], [5, 0, 2], [0, 2, 2]], np.float32)
    three = S.MeshScene(tv, np.arange(9, dtype=np.int32).reshape(3, 3), device=device)
    g = torch.Generator(device=device)
    g.manual_seed(5)
    N = 20000
    pts = S.sample_surface(three, N, generator=g)
    z = pts[:, 2].cpu().numpy()
    assert np.isin(z, (0.0, 1.0, 2.0)).all()
    for k, share in enumerate((1 / 8, 2 / 8, 5 / 8)):
        assert abs(int((z == k).sum()) - N * share) <= 5.0 * np.sqrt(N * share * (1 - share)), (k, int((z == k).sum()))
    with pytest.raises(ValueError, match="uniforms"):
        S.sample_surface(three, 4, uniforms=torch.zeros(3, 3, dtype=torch.float64))


def check_round_trip(device):
    """render -> judge.depth_cloud puts every pixel on a wall.  depth_cloud truncates z to a millimetre, which moves the point along its ray
    d = (dx, dy, 1) z by less than 1 mm x |d|; at 64 x 48 with f = 48, |d| <= sqrt(1 + (33/48)^2 + (25/48)^2) = 1.32, so the point stays within
    1.32 mm of the wall plane it was on; float32 adds micrometres at room coordinates.  Bound: 1.5 mm."""
    from activesplat_amd import judge as J
    mesh = flat_room()
    scene = S.MeshScene(*mesh, device=device)
    W, H = 64, 48
    k4 = k_for(W, H, 48.0)
    for w2c in GENERIC_POSES:
        _, depth, tri_id = S.render_mesh(scene, k4, w2c, W, H, NEAR)
        assert bool((tri_id >= 0).all())
        pts, valid = J.depth_cloud(depth, k4, np.linalg.inv(w2c))
        p = pts.cpu().numpy().astype(np.float64)
        assert bool(valid.bool().all())
        d = np.min(np.stack([np.abs(p[:, ax] - bound) for ax in range(3) for bound in ROOM[ax]], 1), 1)
        print("round trip: farthest point from a wall plane", d.max())
        assert d.max() <= 1.5e-3, d.max()


def _quat(rot):
    """(w, x, y, z) of a rotation matrix"""
    w = np.sqrt(max(0.0, 1.0 + rot[0, 0] + rot[1, 1] + rot[2, 2])) / 2
    assert w > 0.3
    return np.array([w, (rot[2, 1] - rot[1, 2]) / (4 * w), (rot[0, 2] - rot[2, 0]) / (4 * w), (rot[1, 0] - rot[0, 1]) / (4 * w)], np.float32)


def sensor_poses(n=6):
    """X_WV in the simulator's convention (y up, the camera looks along its -z): 0.25 m forward and a 10 degree turn per frame"""
    out, position, yaw = [], np.array([0.0, 0.0, 1.5]), 0.0
    for _ in range(n):
        c, s = np.cos(yaw), np.sin(yaw)
        X = np.eye(4)
        X[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        X[:3, 3] = position
        out.append(X)
        position = position + 0.25 * (X[:3, :3] @ np.array([0.0, 0.0, -1.0]))
        yaw += np.deg2rad(10.0)
    return out


def run_sequence(device, through_host, judge=False, device_ingest=True, frames=6):
    from activesplat_amd import frames as FR
    from activesplat_amd import judge as J
    from activesplat_amd import synthetic as syn
    from activesplat_amd.mapper import SplatMapper
    W, H = 64, 48
    room = S.MeshScene(*flat_room(), device=device)
    K = syn.intrinsics(W, H, fx=32.0, fy=32.0)
    sensor = S.MeshSensor(room, K, W, H)
    poses = sensor_poses(frames)
    mp = SplatMapper(K, W, H, config=dict(step_num=len(poses), densify_downscale_factor=2, device_ingest=device_ingest), device=device)
    if judge:
        samples = S.sample_surface(room.transformed(sensor.w2c(poses[0])), 2000, uniforms=torch.from_numpy(np.random.RandomState(3).uniform(size=(2000, 3))))
        mp.judge = J.CompletionJudge(samples)
    first = None
    for fid, X in enumerate(poses):
        gt_w2c, first = FR.gt_w2c_from_pose(X, first)
        quat, position = _quat(gt_w2c[:3, :3].astype(np.float64)), gt_w2c[:3, 3]
        if through_host:
            image, depth = sensor.frame(X)
            mp.run_raw(image.cpu().numpy(), depth.cpu().numpy(), X, fid, quat, position)
        else:
            mp.run_sensor(sensor, X, fid, quat, position)
    return mp


def check_mapper(device):
    from tests.ingest_cases import same_bits
    a = run_sequence(device, through_host=True)
    b = run_sequence(device, through_host=False, judge=True)
    assert b._ingest is not None and b._ingest.sizes == [(64, 48), (32, 24)]
    assert [k["id"] for k in a.keyframe_list] == [k["id"] for k in b.keyframe_list] and len(a.keyframe_list) >= 2
    for ka, kb in zip(a.keyframe_list, b.keyframe_list):
        assert torch.equal(ka["color"], kb["color"]) and same_bits(ka["depth"], kb["depth"]), ka["id"]
        assert float(ka["depth"].min()) > 0.0 and float(ka["color"].max()) > 0.1                # a room was seen, not an empty frame
    assert len(a.gt_w2c_all_frames) == len(b.gt_w2c_all_frames) == 6
    for ga, gb in zip(a.gt_w2c_all_frames, b.gt_w2c_all_frames):
        assert same_bits(ga, gb)
    assert (b.densify_cam.image_width, b.densify_cam.image_height) == (32, 24)
    # run_sensor takes the device ingest also with the key off (two frames are enough to see it)
    c = run_sequence(device, through_host=False, device_ingest=False, frames=2)
    assert c._ingest is not None and len(c.gt_w2c_all_frames) == 2 and same_bits(c.gt_w2c_all_frames[1], b.gt_w2c_all_frames[1])
    assert torch.equal(c.keyframe_list[0]["color"], b.keyframe_list[0]["color"]) and same_bits(c.keyframe_list[0]["depth"], b.keyframe_list[0]["depth"])
    ratio = b.judge.rows()[:, 1]
    print("completion ratio per frame:", ratio.tolist())
    assert len(ratio) == 6 and (np.diff(ratio) >= 0).all() and ratio[-1] > ratio[0] > 0.0
