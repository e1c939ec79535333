"""Shared checks of the textured mesh sensor (activesplat_amd/sensor.py; gs_texture_layout, gs_texture_build_mips, gs_mesh_render_textured): run on
the host-emulated kernels by tests/test_mesh_textures.py and on the MI355X by tests/test_gpu_mesh_textures.py.

Expected values
* `restate_mips`: the mip chain of include/gsplat_hip.h in numpy integers; the pool read back must equal it word for word.
* `restate_texture(...)`: the per-pixel rule of include/gsplat_hip.h (gs_mesh_render_textured) in numpy, in float64 (the expected colour c64, BEFORE
  rounding) and in float32 (c32, only to measure how far a float32 evaluation of the same rule lies from the float64 one).  Both take tri_id from
  `mesh_cases.restate(..., float64)`.  Nothing from the code under test goes into them.
* The tolerance of a case is tol = max(1e-3, 8 max|c32 - c64|) over the unflagged textured pixels: the factor 8 is mesh_cases' allowance for fused
  multiply-adds and another summation order in the kernel; the floor only keeps a case whose float32 restatement happens to agree exactly from
  demanding bit equality.  On unflagged pixels a textured pixel must satisfy |u8 - c64| <= 0.5 + tol and an untextured one must equal
  `render_mesh` of the same mesh without textures; on flagged pixels (mesh_cases' edge-critical pixels) only hit-or-not is compared.
* Asserted on the reference alone, before anything is compared: tol <= 0.05, and the flagged share within mesh_cases' caps (1 % at generic
  poses, 5 % at the axis pose).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from activesplat_amd import _lib
from activesplat_amd import rasterizer as R
from activesplat_amd import sensor as S
from tests import mesh_cases as mc

GS_EINVAL = 1
REPEAT, CLAMP, MIRROR = 0, 1, 2

# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------------


def restate_mips(image):
    """uint8 [h, w, 3] -> the list of levels, level 0 first, by the integer rule"""
    levels = [np.asarray(image, np.uint8).astype(np.int64)]
    while max(levels[-1].shape[:2]) > 1:
        t = levels[-1]
        h, w = t.shape[:2]
        j0, i0 = 2 * np.arange(max(1, h >> 1)), 2 * np.arange(max(1, w >> 1))
        j1, i1 = np.minimum(j0 + 1, h - 1), np.minimum(i0 + 1, w - 1)
        levels.append((t[j0][:, i0] + t[j0][:, i1] + t[j1][:, i0] + t[j1][:, i1] + 2) >> 2)
    return [lv.astype(np.uint8) for lv in levels]


def restate_pool(textures):
    """the whole pool as packed RGBX words, and (offset, w, h) per texture and level"""
    words, where, at = [], [], 0
    for image, _, _ in textures:
        where.append([])
        for lv in restate_mips(image):
            lv = lv.astype(np.uint32)
            words.append((lv[..., 0] | (lv[..., 1] << 8) | (lv[..., 2] << 16)).reshape(-1))
            where[-1].append((at, lv.shape[1], lv.shape[0]))
            at += lv.shape[0] * lv.shape[1]
    return np.concatenate(words).astype(np.uint32), where


def _wrap(i, n, mode):
    if mode == CLAMP:
        return np.clip(i, 0, n - 1)
    if mode == REPEAT:
        return np.mod(i, n)
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def _sample(level, ws, wt, u, v, f):
    """the bilinear sample of one level (uint8 [h, w, 3]) at (u, v) [n] in dtype f -> [n, 3]"""
    h, w = level.shape[:2]
    s, t = u * f(w) - f(0.5), v * f(h) - f(0.5)
    fi, fj = np.floor(s), np.floor(t)
    al, be = (s - fi)[:, None], (t - fj)[:, None]
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    i0, i1, j0, j1 = _wrap(i, w, ws), _wrap(i + 1, w, ws), _wrap(j, h, wt), _wrap(j + 1, h, wt)
    T = level.astype(f)
    top = (f(1) - al) * T[j0, i0] + al * T[j0, i1]
    bot = (f(1) - al) * T[j1, i0] + al * T[j1, i1]
    return (f(1) - be) * top + be * bot


def restate_texture(vertices, triangles, uvs, tri_texture, textures, k4, w2c, W, H, tri_id, dtype=np.float64):
    """the texture rule in `dtype` on the winners `tri_id` [H, W] -> dict(color [H, W, 3] of `dtype` BEFORE rounding (0 where the pixel is not
    textured), textured [H, W] bool, lam [H, W] (the level of detail))"""
    f = dtype
    v = np.asarray(vertices, np.float32).astype(f)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    uv = np.asarray(uvs, np.float32).astype(f)
    tt = np.asarray(tri_texture, np.int64)
    m = np.asarray(w2c, np.float64)[:3].astype(np.float32).astype(f)
    fx, fy, cx, cy = (f(np.float32(a)) for a in k4)
    p = np.stack([m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1] + m[r, 2] * v[:, 2] + m[r, 3] for r in range(3)], 1)
    safe = np.maximum(tri_id, 0)
    tex = np.where(tri_id >= 0, tt[safe] if len(tt) else -1, -1)
    textured = (tex >= 0) & (tex < len(textures))
    ys, xs = np.nonzero(textured)
    color = np.zeros((H, W, 3), f)
    lam_image = np.zeros((H, W), f)
    if len(ys) == 0:
        return dict(color=color, textured=textured, lam=lam_image)
    t = tri[tri_id[ys, xs]]

    def normal(i, j):
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        a, b = p[lo], p[hi]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        return np.where((i > j)[:, None], -n, n)
    nU, nV, nW = normal(t[:, 1], t[:, 2]), normal(t[:, 2], t[:, 0]), normal(t[:, 0], t[:, 1])
    with np.errstate(all="ignore"):
        q = []
        for ox, oy in ((0, 0), (1, 0), (0, 1)):
            dx, dy = ((xs + ox).astype(f) - cx) / fx, ((ys + oy).astype(f) - cy) / fy
            U, V, Wt = (dx * n[:, 0] + dy * n[:, 1] + n[:, 2] for n in (nU, nV, nW))
            Ssum = U + V + Wt
            q.append((U[:, None] * uv[t[:, 0]] + V[:, None] * uv[t[:, 1]] + Wt[:, None] * uv[t[:, 2]]) / Ssum[:, None])
        out = np.zeros((len(ys), 3), f)
        lam_out = np.zeros(len(ys), f)
        mine = tex[ys, xs]
        for k, (image, ws, wt) in enumerate(textures):
            sel = np.nonzero(mine == k)[0]
            if len(sel) == 0:
                continue
            levels = restate_mips(image)
            L = len(levels)
            h0, w0 = levels[0].shape[:2]
            size = np.array([w0, h0]).astype(f)
            q0 = q[0][sel]
            ex, ey = (q[1][sel] - q0) * size, (q[2][sel] - q0) * size
            rho = np.maximum(np.sqrt(ex[:, 0] * ex[:, 0] + ex[:, 1] * ex[:, 1]), np.sqrt(ey[:, 0] * ey[:, 0] + ey[:, 1] * ey[:, 1]))   # (np.maximum keeps a NaN)
            lam = np.where(rho <= 1, f(0), np.where(np.isfinite(rho), np.minimum(np.log2(np.where(rho > 1, rho, f(2))), f(L - 1)), f(L - 1))).astype(f)
            wild = ~(np.isfinite(q0).all(1) & (np.abs(q0) <= 2.0 ** 20).all(1))
            u, vv = np.where(wild, f(0), q0[:, 0]), np.where(wild, f(0), q0[:, 1])
            l0 = np.floor(lam)
            fr = (lam - l0)[:, None]
            c = np.zeros((len(sel), 3), f)
            for level in range(L):
                at = np.nonzero((l0 == level) & ~wild)[0]
                if len(at):
                    nxt = min(level + 1, L - 1)
                    c[at] = (f(1) - fr[at]) * _sample(levels[level], ws, wt, u[at], vv[at], f) + fr[at] * _sample(levels[nxt], ws, wt, u[at], vv[at], f)
            c[wild] = levels[L - 1][0, 0].astype(f)
            out[sel], lam_out[sel] = c, lam
    color[ys, xs] = out
    lam_image[ys, xs] = lam_out
    return dict(color=color, textured=textured, lam=lam_image)


# ---- references, computed once ----------------------------------------------------------------------------------------------------------------

_reference = {}


def reference(key, mesh, uvs, tri_texture, textures, k4, w2c, W, H, near):
    """(mesh_cases' float64 restatement, c64 dict, tol) of a case, computed once per session, shared and read-only"""
    if key not in _reference:
        v, t, c = mesh
        r64 = mc.restate(v, t, c, k4, w2c, W, H, near, np.float64)
        c64 = restate_texture(v, t, uvs, tri_texture, textures, k4, w2c, W, H, r64["tri_id"], np.float64)
        c32 = restate_texture(v, t, uvs, tri_texture, textures, k4, w2c, W, H, r64["tri_id"], np.float32)
        ok = c64["textured"] & ~r64["flagged"]
        worst = float(np.abs(c32["color"].astype(np.float64) - c64["color"])[ok].max()) if ok.any() else 0.0
        c64["fp32_worst"] = worst
        for d in (r64, c64):
            for a in d.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _reference[key] = (r64, c64, max(1e-3, 8.0 * worst))
    return _reference[key]


def render(scene, k4, w2c, W, H, near):
    color, depth, tri_id = S.render_mesh(scene, k4, w2c, W, H, near)
    assert color.shape == (H, W, 3) and color.dtype == torch.uint8 and depth.shape == (H, W) and depth.dtype == torch.float32
    assert tri_id.shape == (H, W) and tri_id.dtype == torch.int32
    return color.cpu().numpy(), depth.cpu().numpy(), tri_id.cpu().numpy()


def compare(what, got, plain, ref, cap):
    """got: the textured render, plain: render_mesh of the same mesh without textures, ref: reference(...)"""
    r64, c64, tol = ref
    color, depth, tri_id = got
    flagged, textured = r64["flagged"], c64["textured"]
    share = float(flagged.mean())
    lam = c64["lam"][textured & ~flagged]
    print(f"{what}: flagged {100 * share:.3f} %  numpy-fp32 worst |c32 - c64| {c64['fp32_worst']:.2e}  tol {tol:.2e}  textured pixels {int(textured.sum())}  "
          f"lambda {lam.min() if lam.size else 0:.2f} .. {lam.max() if lam.size else 0:.2f}  magnified {100 * float((lam == 0).mean()) if lam.size else 0:.0f} %")
    assert tol <= 0.05, (what, "tolerance", tol)
    assert share <= cap, (what, "flagged share", share)
    # depth and tri_id are gs_mesh_render's bits everywhere
    assert np.array_equal(depth.view(np.int32), plain[1].view(np.int32)) and np.array_equal(tri_id, plain[2]), (what, "depth / tri_id")
    hit = r64["tri_id"] >= 0
    assert np.array_equal(tri_id >= 0, hit), (what, "hit mask")
    ok = ~flagged
    assert np.array_equal(tri_id[ok], r64["tri_id"][ok]), (what, "tri_id")
    plainly = ok & ~textured
    assert np.array_equal(color[plainly], plain[0][plainly]), (what, "untextured pixels")
    err = np.abs(color.astype(np.float64) - c64["color"])[ok & textured]
    print(f"{what}: kernel worst |u8 - c64| {err.max() if err.size else 0:.4f} (allowed {0.5 + tol:.4f})")
    assert (err <= 0.5 + tol).all(), (what, "colour", float(err.max()), 0.5 + tol)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------

def random_textures(seed=5):
    """32 x 32, 17 x 9 (w x h), 64 x 64 and 1 x 1 (L = 1), random texels; every wrap mode occurs on both axes"""
    rng = np.random.RandomState(seed)
    im = lambda w, h: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)  # noqa: E731
    return [(im(32, 32), REPEAT, MIRROR), (im(17, 9), CLAMP, REPEAT), (im(64, 64), MIRROR, CLAMP), (im(1, 1), REPEAT, REPEAT)]


def random_textured_scene(seed=0):
    """mesh_cases.random_scene() with uvs uniform in [-1, 2] and a texture index random in -1 .. 3 per triangle"""
    mesh = mc.random_scene(seed)
    rng = np.random.RandomState(seed + 100)
    uvs = rng.uniform(-1.0, 2.0, (len(mesh[0]), 2)).astype(np.float32)
    textures = random_textures()
    tri_texture = rng.randint(-1, len(textures), len(mesh[1])).astype(np.int32)
    return mesh, uvs, tri_texture, textures


def scene_of(device, mesh, uvs, tri_texture, textures):
    return S.MeshScene(*mesh, device=device, uvs=uvs, textures=textures, tri_texture=tri_texture)


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------

def check_mip_chains(device):
    rng = np.random.RandomState(2)
    textures = [(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), REPEAT, REPEAT) for w, h in ((32, 32), (17, 9), (5, 1), (1, 1), (64, 64))]
    v = np.zeros((3, 3), np.float32)
    scene = S.MeshScene(v, np.array([[0, 1, 2]], np.int32), device=device, uvs=np.zeros((3, 2), np.float32), textures=textures)
    want, where = restate_pool(textures)
    assert [len(w) for w in where] == [6, 5, 3, 1, 7]
    assert scene.pool_texels == len(want)
    for k, levels in enumerate(where):
        d = scene._h_table[k]
        assert d.levels == len(levels) and [int(d.level_offset[l]) for l in range(len(levels))] == [at for at, _, _ in levels]
        assert all(int(d.level_offset[l]) == 0 for l in range(len(levels), _lib.TEXTURE_MAX_LEVELS))
    got = scene.texture_pool.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(scene.texture_level(1, 2).cpu().numpy(), restate_mips(textures[1][0])[2])


def check_random_scene(device):
    mesh, uvs, tri_texture, textures = random_textured_scene()
    scene = scene_of(device, mesh, uvs, tri_texture, textures)
    bare = S.MeshScene(*mesh, device=device)
    for (W, H), poses in (((64, 48), mc.GENERIC_POSES + (mc.AXIS_POSE,)), ((37, 29), mc.GENERIC_POSES[:1])):
        k4 = mc.k_for(W, H, 40.0)
        for i, w2c in enumerate(poses):
            ref = reference(("random", W, H, i), mesh, uvs, tri_texture, textures, k4, w2c, W, H, mc.NEAR)
            seen = set(np.unique(np.asarray(tri_texture)[ref[0]["tri_id"][ref[0]["tri_id"] >= 0]]).tolist())
            assert W != 64 or seen == {-1, 0, 1, 2, 3}, seen                                   # every texture and the vertex colours are seen
            compare(f"random textured scene {W} x {H} pose {i}", render(scene, k4, w2c, W, H, mc.NEAR), render(bare, k4, w2c, W, H, mc.NEAR), ref,
                    0.05 if i == 3 else 0.01)


def check_worked_by_hand(device):
    """(a) Pure magnification.  One triangle (-1, -1), (3, -1), (-1, 3) at z = 2 seen through f = 1, centre (1, 1), 3 x 3 pixels (the case of
    tests/test_mesh_sensor.py): pixel (1, 1) is the point (0, 0) with weights (1/2, 1/4, 1/4).  With uvs (0, 0), (1/2, 0), (0, 1/2) it has
    q = (1/8, 1/8), and one pixel step moves q by 1/4, i.e. by half a texel of a 2 x 2 texture: rho = 1/2, lambda = 0.  At level 0
    s = t = 1/8 * 2 - 1/2 = -1/4: i = j = -1, alpha = beta = 3/4, and REPEAT wraps -1 to 1.  So
      c = 1/4 (1/4 T[1][1] + 3/4 T[1][0]) + 3/4 (1/4 T[0][1] + 3/4 T[0][0]) = (T[1][1] + 3 T[1][0] + 3 T[0][1] + 9 T[0][0]) / 16.
    With T[0][0] = (160, 0, 0), T[0][1] = (16, 64, 0), T[1][0] = (32, 128, 0), T[1][1] = (240, 0, 255):
      R = (240 + 96 + 48 + 1440) / 16 = 114, G = (384 + 192) / 16 = 36, B = 255 / 16 = 15.9375 -> 16.
    (b) Exact minification.  A quad (-2, -2) .. (2, 2) at z = 1 seen through f = 4, centre (3.5, 3.5), 8 x 8 pixels, uv = (X + 2, Y + 2) / 4 and a
    64 x 64 texture of constant 4 x 4 blocks: pixel x has u = ((x - 3.5) / 4 + 2) / 4 = (x + 4.5) / 16; a pixel step is 1/16 = 4 texels, so
    rho = 4 and lambda = 2 exactly (every number is dyadic and S = 16).  Level 2 has 16 x 16 texels, each the mean of one constant block,
    i.e. that block's colour; s = 16 u - 1/2 = x + 4 gives i = x + 4, alpha = 0 (likewise rows): pixel (x, y) shows block (y + 4, x + 4) exactly.
    (Should an evaluation land an ulp below, i = x + 3 with alpha = 1 - ulp, or lambda = 2 - ulp: the rounded level is the same.)"""
    v = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    uv = np.array([[0, 0], [0.5, 0], [0, 0.5]], np.float32)
    T = np.array([[[160, 0, 0], [16, 64, 0]], [[32, 128, 0], [240, 0, 255]]], np.uint8)
    k4 = (1.0, 1.0, 1.0, 1.0)
    r = mc.restate(v, t, np.zeros((3, 3), np.uint8), k4, np.eye(4), 3, 3, 0.05)
    c64 = restate_texture(v, t, uv, [0], [(T, REPEAT, REPEAT)], k4, np.eye(4), 3, 3, r["tri_id"])
    assert c64["color"][1, 1].tolist() == [114.0, 36.0, 15.9375] and c64["lam"][1, 1] == 0 and not r["flagged"][1, 1]
    color, _, tri_id = render(S.MeshScene(v, t, device=device, uvs=uv, textures=[T]), k4, np.eye(4), 3, 3, 0.05)
    assert tri_id[1, 1] == 0 and color[1, 1].tolist() == [114, 36, 16], color[1, 1]
    assert (color[tri_id < 0] == 0).all()
    # (b)
    rng = np.random.RandomState(8)
    blocks = rng.randint(0, 256, (16, 16, 3)).astype(np.uint8)
    image = np.repeat(np.repeat(blocks, 4, 0), 4, 1)
    v = np.array([[-2, -2, 1], [2, -2, 1], [2, 2, 1], [-2, 2, 1]], np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = ((v[:, :2] + 2) / 4).astype(np.float32)
    k4 = (4.0, 4.0, 3.5, 3.5)
    r = mc.restate(v, t, np.zeros((4, 3), np.uint8), k4, np.eye(4), 8, 8, 0.05)
    assert (r["tri_id"] >= 0).all()
    c64 = restate_texture(v, t, uv, [0, 0], [(image, CLAMP, CLAMP)], k4, np.eye(4), 8, 8, r["tri_id"])
    assert (c64["lam"] == 2).all() and np.array_equal(c64["color"], blocks[4:12, 4:12].astype(np.float64))
    color, _, tri_id = render(S.MeshScene(v, t, device=device, uvs=uv, textures=[(image, CLAMP, CLAMP)]), k4, np.eye(4), 8, 8, 0.05)
    assert (tri_id >= 0).all() and np.array_equal(color, blocks[4:12, 4:12])


def check_grazing(device):
    """mesh_cases.crossing_scene(): the floor (two triangles of 40 m x 40 m passing under the camera) carries a 64 x 64 REPEAT texture tiled once
    per metre; towards the horizon a pixel step covers more than the whole texture and lambda reaches L - 1 = 6"""
    mesh = mc.crossing_scene()
    v, t, _ = mesh
    uvs = v[:, [0, 2]].astype(np.float32).copy()
    textures = [(np.random.RandomState(6).randint(0, 256, (64, 64, 3)).astype(np.uint8), REPEAT, REPEAT)]
    tri_texture = np.array([0, 0, -1, -1], np.int32)
    scene = scene_of(device, mesh, uvs, tri_texture, textures)
    bare = S.MeshScene(*mesh, device=device)
    W, H = 48, 40
    k4 = mc.k_for(W, H, 24.0)
    for i, w2c in enumerate((mc.pose(0.11, 0.07, 0.03, (0.0, 0.0, 0.0)), mc.pose(0.4, 0.45, -0.2, (0.3, -0.2, 0.1)))):
        ref = reference(("grazing", i), mesh, uvs, tri_texture, textures, k4, w2c, W, H, mc.NEAR)
        lam = ref[1]["lam"][ref[1]["textured"] & ~ref[0]["flagged"]]
        assert lam.size > 200 and lam.max() == 6.0 and lam.min() < 5.0, (lam.size, lam.min(), lam.max())
        compare(f"grazing floor pose {i}", render(scene, k4, w2c, W, H, mc.NEAR), render(bare, k4, w2c, W, H, mc.NEAR), ref, 0.01)


def check_identity(device):
    """depth and tri_id are those of the mesh without textures, and so is the colour wherever tri_texture is -1"""
    mesh, uvs, tri_texture, textures = random_textured_scene()
    W, H = 64, 48
    k4, w2c = mc.k_for(W, H, 40.0), mc.GENERIC_POSES[1]
    plain = render(S.MeshScene(*mesh, device=device), k4, w2c, W, H, mc.NEAR)
    got = render(scene_of(device, mesh, uvs, tri_texture, textures), k4, w2c, W, H, mc.NEAR)
    assert np.array_equal(got[1].view(np.int32), plain[1].view(np.int32)) and np.array_equal(got[2], plain[2])
    tex = np.where(got[2] >= 0, tri_texture[np.maximum(got[2], 0)], -1)
    assert (tex == -1).sum() > 100 and np.array_equal(got[0][tex == -1], plain[0][tex == -1])
    assert not np.array_equal(got[0][tex >= 0], plain[0][tex >= 0])                            # (and the textured pixels did change)
    # through the C ABI a value outside 0 .. num_textures - 1 means the same as -1 (MeshScene refuses such values, so they are put in behind it)
    wild = scene_of(device, mesh, uvs, tri_texture, textures)
    far = np.where(tri_texture == 0, np.int32(-2 ** 31), np.where(tri_texture == 1, np.int32(4), np.where(tri_texture == 2, np.int32(2 ** 31 - 1), tri_texture)))
    wild.tri_texture = torch.from_numpy(far.astype(np.int32)).to(wild.tri_texture.device)
    got2 = render(wild, k4, w2c, W, H, mc.NEAR)
    assert np.array_equal(got2[0][tex != 3], plain[0][tex != 3]) and np.array_equal(got2[0][tex == 3], got[0][tex == 3])
    assert np.array_equal(got2[1].view(np.int32), plain[1].view(np.int32)) and np.array_equal(got2[2], plain[2])


PAD = 4096


def _padded(t, device):
    """a copy of `t` on the device with PAD bytes of 0xAB in front and behind -> (view, whole buffer, number of payload bytes)"""
    raw = t.detach().contiguous().reshape(-1).view(torch.uint8)
    n = raw.numel()
    whole = torch.full((2 * PAD + n,), 0xAB, dtype=torch.uint8, device=device)
    whole[PAD:PAD + n] = raw.to(device)
    return whole[PAD:PAD + n].view(t.dtype).view(t.shape), whole, n


def _pads_intact(whole, n):
    return bool((whole[:PAD] == 0xAB).all()) and bool((whole[PAD + n:] == 0xAB).all())


def _abi_call(device, scene, k4, w2c, W, H, near, capacity=4096, guard=4096, textured=True, **over):
    """gs_mesh_render_textured (or gs_mesh_render) with pads around the scratch, the colour image, the pool and the device table ->
    (rc, (color, depth, tri_id), every pad intact and pool / table unchanged)"""
    lib = _lib.get()
    T = scene.num_triangles
    layout = _lib.GsMeshLayout()
    assert lib.gs_mesh_render_layout(T, W, H, capacity, C.byref(layout)) == 0
    n = int(layout.total_bytes)
    buf = torch.full((n + guard,), 0xAB, dtype=torch.uint8, device=device)
    depth = torch.full((H, W), -7.0, dtype=torch.float32, device=device)
    tri_id = torch.full((H, W), -7, dtype=torch.int32, device=device)
    color, color_whole, color_n = _padded(torch.full((H, W, 3), 7, dtype=torch.uint8), device)
    pool, pool_whole, pool_n = _padded(scene.texture_pool, device)
    table, table_whole, table_n = _padded(scene.texture_table, device)
    pool_before, table_before = pool_whole.clone(), table_whole.clone()
    counts = torch.zeros(2, dtype=torch.int32, device=device)
    k = np.asarray(k4, np.float32).copy()
    m = np.ascontiguousarray(np.asarray(w2c, np.float64)[:3].reshape(12), dtype=np.float32)
    h_table = (_lib.GsTextureDesc * scene.num_textures)()
    C.memmove(h_table, scene._h_table, C.sizeof(h_table))
    fp = C.POINTER(C.c_float)
    a = dict(num_vertices=scene.num_vertices, vertices=R._ptr(scene.vertices), num_triangles=T, triangles=R._ptr(scene.triangles),
             colors=R._ptr(scene.vertex_colors), k=k.ctypes.data_as(fp), m=m.ctypes.data_as(fp), near_z=float(near), width=W, height=H, scratch=R._ptr(buf),
             capacity=capacity, depth=R._ptr(depth), tri_id=R._ptr(tri_id), color=R._ptr(color), counts=R._ptr(counts), uvs=R._ptr(scene.uvs),
             tri_texture=R._ptr(scene.tri_texture), num_textures=scene.num_textures, h_table=h_table, table=R._ptr(table), pool=R._ptr(pool),
             pool_texels=scene.pool_texels)
    edit = over.pop("edit", None)
    if edit is not None:
        edit(h_table)
    a.update(over)
    first = (a["num_vertices"], a["vertices"], a["num_triangles"], a["triangles"], a["colors"], a["k"], a["m"], a["near_z"], a["width"], a["height"],
             a["scratch"], a["capacity"], a["depth"], a["tri_id"], a["color"], a["counts"])
    stream = _lib.stream_ptr(torch.device(device))
    if textured:
        rc = lib.gs_mesh_render_textured(*first, a["uvs"], a["tri_texture"], a["num_textures"], a["h_table"], a["table"], a["pool"], a["pool_texels"], stream)
    else:
        rc = lib.gs_mesh_render(*first, stream)
    intact = bool((buf[n:] == 0xAB).all()) and _pads_intact(color_whole, color_n) and torch.equal(pool_whole, pool_before) and torch.equal(table_whole, table_before)
    return rc, (color.cpu().numpy().copy(), depth.cpu().numpy(), tri_id.cpu().numpy()), intact


def check_guarded_abi(device):
    lib = _lib.get()
    mesh, uvs, tri_texture, textures = random_textured_scene()
    scene = scene_of(device, mesh, uvs, tri_texture, textures)
    W, H = 37, 29
    k4, w2c = mc.k_for(W, H, 40.0), mc.GENERIC_POSES[0]
    rc, got, intact = _abi_call(device, scene, k4, w2c, W, H, mc.NEAR)
    assert rc == 0 and intact
    via_python = render(scene, k4, w2c, W, H, mc.NEAR)
    for x, y in zip(got, via_python):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # num_textures == 0 equals gs_mesh_render, with everything texture-related null
    rc, plain, intact = _abi_call(device, scene, k4, w2c, W, H, mc.NEAR, textured=False)
    assert rc == 0 and intact
    rc, zero, intact = _abi_call(device, scene, k4, w2c, W, H, mc.NEAR, num_textures=0, uvs=None, tri_texture=None, h_table=None, table=None, pool=None, pool_texels=0)
    assert rc == 0 and intact
    for x, y in zip(zero, plain):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not np.array_equal(got[0], plain[0])
    # a capacity that is too small clears the outputs, textured or not
    rc, short, intact = _abi_call(device, scene, k4, w2c, W, H, mc.NEAR, capacity=1)
    assert rc == 0 and intact and (short[2] == -1).all() and (short[1] == 0).all() and (short[0] == 0).all()
    # refusals: GS_EINVAL, and nothing is written
    untouched = lambda outs: (outs[1] == -7).all() and (outs[2] == -7).all() and (outs[0] == 7).all()  # noqa: E731

    def set_field(index, name, value):
        def edit(h_table):
            setattr(h_table[index], name, value)
        return edit

    def set_offset(h_table):
        h_table[1].level_offset[1] += 1
    for over, text in ((dict(uvs=None), b"null"), (dict(tri_texture=None), b"null"), (dict(h_table=None), b"null"), (dict(table=None), b"null"),
                       (dict(pool=None), b"null"), (dict(num_textures=-1), b"num_textures"),
                       (dict(edit=set_field(0, "wrap_s", 3)), b"wrap mode"), (dict(edit=set_field(2, "wrap_t", -1)), b"wrap mode"),
                       (dict(edit=set_field(1, "width", 0)), b"texture size"), (dict(edit=set_field(1, "height", 16385)), b"texture size"),
                       (dict(edit=set_field(3, "width", -5)), b"texture size"), (dict(edit=set_field(0, "levels", 5)), b"gs_texture_layout"),
                       (dict(edit=set_offset), b"gs_texture_layout"), (dict(pool_texels=scene.pool_texels - 1), b"pool_texels"),
                       (dict(vertices=None), b"null"), (dict(color=None), b"null"), (dict(width=0), b"image size"), (dict(near_z=0.0), b"near")):
        rc, outs, intact = _abi_call(device, scene, k4, w2c, W, H, mc.NEAR, **over)
        assert rc == GS_EINVAL and text in lib.gs_last_error(), (over, rc, lib.gs_last_error())
        assert untouched(outs) and intact, over
    # the layout call and the mip build refuse the same tables, before anything is written
    table = (_lib.GsTextureDesc * 2)()
    texels = C.c_uint64(77)
    for w, h, ws, wt in ((0, 4, 0, 0), (4, 16385, 0, 0), (4, 4, 3, 0), (4, 4, 0, -1)):
        table[0].width, table[0].height, table[0].wrap_s, table[0].wrap_t = 4, 4, 0, 0
        table[1].width, table[1].height, table[1].wrap_s, table[1].wrap_t = w, h, ws, wt
        table[0].levels = table[1].levels = -9
        assert lib.gs_texture_layout(2, table, C.byref(texels)) == GS_EINVAL and texels.value == 77 and table[0].levels == -9, (w, h, ws, wt)
    assert lib.gs_texture_layout(-1, table, C.byref(texels)) == GS_EINVAL and lib.gs_texture_layout(1, None, C.byref(texels)) == GS_EINVAL
    assert lib.gs_texture_layout(1, table, None) == GS_EINVAL
    assert lib.gs_texture_layout(0, None, C.byref(texels)) == 0 and texels.value == 0
    pool, pool_whole, pool_n = _padded(scene.texture_pool, device)
    before = pool_whole.clone()
    stream = _lib.stream_ptr(torch.device(device))
    h_table = (_lib.GsTextureDesc * scene.num_textures)()
    C.memmove(h_table, scene._h_table, C.sizeof(h_table))
    h_table[2].wrap_s = 7
    assert lib.gs_texture_build_mips(scene.num_textures, h_table, R._ptr(scene.texture_table), R._ptr(pool), scene.pool_texels, stream) == GS_EINVAL
    assert lib.gs_texture_build_mips(scene.num_textures, scene._h_table, R._ptr(scene.texture_table), None, scene.pool_texels, stream) == GS_EINVAL
    assert lib.gs_texture_build_mips(scene.num_textures, scene._h_table, R._ptr(scene.texture_table), R._ptr(pool), scene.pool_texels + 1, stream) == GS_EINVAL
    assert lib.gs_texture_build_mips(-1, scene._h_table, R._ptr(scene.texture_table), R._ptr(pool), scene.pool_texels, stream) == GS_EINVAL
    assert torch.equal(pool_whole, before)
    # a well-formed build on the padded copy rewrites the levels above 0 with the same words and leaves the pads alone
    pool[int(scene._h_table[0].level_offset[1]):int(scene._h_table[1].level_offset[0])] = 0
    assert lib.gs_texture_build_mips(scene.num_textures, scene._h_table, R._ptr(scene.texture_table), R._ptr(pool), scene.pool_texels, stream) == 0
    assert torch.equal(pool_whole, before)


def check_repeatable(device):
    mesh, uvs, tri_texture, textures = random_textured_scene()
    W, H = 64, 48
    k4, w2c = mc.k_for(W, H, 40.0), mc.GENERIC_POSES[2]
    scene = scene_of(device, mesh, uvs, tri_texture, textures)
    a, b = render(scene, k4, w2c, W, H, mc.NEAR), render(scene, k4, w2c, W, H, mc.NEAR)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # the texture list in another order, tri_texture remapped: the same image
    perm = [2, 0, 3, 1]                                                                        # new position -> old index
    new_of_old = np.argsort(perm)
    remapped = np.where(tri_texture >= 0, new_of_old[np.maximum(tri_texture, 0)], -1).astype(np.int32)
    c = render(scene_of(device, mesh, uvs, remapped, [textures[o] for o in perm]), k4, w2c, W, H, mc.NEAR)
    for x, y in zip(a, c):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def check_python_validation(device):
    v, t, c = mc.flat_room()
    uv = np.zeros((len(v), 2), np.float32)
    im = np.zeros((4, 4, 3), np.uint8)
    tt = np.zeros(len(t), np.int32)
    make = lambda **k: S.MeshScene(v, t, c, device=device, **{**dict(uvs=uv, textures=[im], tri_texture=tt), **k})  # noqa: E731
    assert make().num_textures == 1 and S.MeshScene(v, t, c, device=device).num_textures == 0
    assert make(tri_texture=None).tri_texture.tolist() == [0] * len(t)
    assert make(textures=[(torch.from_numpy(im), S.WRAP_CLAMP, S.WRAP_MIRROR)], uvs=torch.from_numpy(uv).double(), tri_texture=tt.astype(np.int64) - 1).num_textures == 1
    with pytest.raises(ValueError, match="need uvs"):
        make(uvs=None)
    with pytest.raises(ValueError, match="need textures"):
        make(textures=None)
    with pytest.raises(ValueError, match="need textures"):
        S.MeshScene(v, t, c, device=device, tri_texture=tt)
    with pytest.raises(TypeError, match="uvs must be floating"):
        make(uvs=uv.astype(np.int32))
    with pytest.raises(ValueError, match=r"uvs must have shape \[8, 2\]"):
        make(uvs=uv[:-1])
    with pytest.raises(ValueError, match="uvs must have shape"):
        make(uvs=np.zeros((len(v), 3), np.float32))
    with pytest.raises(TypeError, match="tri_texture must be of a signed integer"):
        make(tri_texture=tt.astype(np.float32))
    with pytest.raises(ValueError, match=r"tri_texture must have shape \[12\]"):
        make(tri_texture=tt[:-1])
    with pytest.raises(ValueError, match="tri_texture outside -1 .. 0"):
        make(tri_texture=tt + 1)
    with pytest.raises(ValueError, match="tri_texture outside"):
        make(tri_texture=tt - 2)
    with pytest.raises(TypeError, match="texture 0 must be uint8"):
        make(textures=[im.astype(np.float32)])
    with pytest.raises(ValueError, match=r"texture 1 must have shape \[h, w, 3\]"):
        make(textures=[im, np.zeros((4, 4, 4), np.uint8)])
    with pytest.raises(ValueError, match="texture 0 must have shape"):
        make(textures=[np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match="wrap modes"):
        make(textures=[(im, 3, 0)])
    # transformed() shares the texture data
    scene = make()
    moved = scene.transformed(np.eye(4))
    assert moved.texture_pool is scene.texture_pool and moved.uvs is scene.uvs and moved.tri_texture is scene.tri_texture and moved.num_textures == 1


def textured_flat_room(device):
    v, t, c = mc.flat_room()
    rng = np.random.RandomState(12)
    uvs = rng.uniform(0.0, 3.0, (len(v), 2)).astype(np.float32)
    textures = [(rng.randint(0, 256, (32, 32, 3)).astype(np.uint8), REPEAT, REPEAT), (rng.randint(0, 256, (16, 8, 3)).astype(np.uint8), MIRROR, CLAMP)]
    tri_texture = np.array([0, 0, 1, 1, -1, -1, 0, 1, 1, 0, -1, 0], np.int32)
    return S.MeshScene(v, t, c, device=device, uvs=uvs, textures=textures, tri_texture=tri_texture)


def check_sensor_and_mapper(device):
    from activesplat_amd import frames as FR
    from activesplat_amd import synthetic as syn
    from activesplat_amd.mapper import SplatMapper
    W, H = 64, 48
    room = textured_flat_room(device)
    K = syn.intrinsics(W, H, fx=32.0, fy=32.0)
    sensor = S.MeshSensor(room, K, W, H)
    poses = mc.sensor_poses(3)
    image, depth = sensor.frame(poses[0])
    color, depth2, tri_id = S.render_mesh(room, sensor.k4, sensor.w2c(poses[0]), W, H)
    assert torch.equal(image, color) and torch.equal(depth, depth2) and bool((tri_id >= 0).all())
    bare = S.MeshScene(room.vertices, room.triangles, room.vertex_colors, device=device)
    assert not torch.equal(S.render_mesh(bare, sensor.k4, sensor.w2c(poses[0]), W, H)[0], color)    # (the textures are seen)
    mp = SplatMapper(K, W, H, config=dict(step_num=len(poses), densify_downscale_factor=2), device=device)
    first = None
    for fid, X in enumerate(poses):
        gt_w2c, first = FR.gt_w2c_from_pose(X, first)
        mp.run_sensor(sensor, X, fid, mc._quat(gt_w2c[:3, :3].astype(np.float64)), gt_w2c[:3, 3])
    assert len(mp.gt_w2c_all_frames) == 3 and len(mp.keyframe_list) >= 1
    losses = mp.last_losses
    losses = losses() if callable(losses) else losses
    print("losses after three frames:", losses)
    assert losses and all(np.isfinite(x) for x in losses.values()), losses
    assert float(mp.keyframe_list[0]["color"].max()) > 0.1
