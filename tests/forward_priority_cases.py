"""Issue priority of the forward blend's walkers (gs_set_forward_priority) changes the order in which the wavefronts of a SIMD issue and nothing
else: every forward output is bit-identical with the knob off and in every mode.  Shared by the emulated (CPU) and the GPU test file.

The scene is the smallest that reaches blend_forward_streams_kernel<SEG = 0> and its branches: 265 x 250 pixels = 17 x 16 = 272 tiles (more than
the 256 of the few-tile kernels) with ragged right and bottom tiles, about 3000 Gaussians, and
  * DENSE tile: a list of at least 200 entries (three or more 64-entry chunks) whose pixels saturate at different depths;
  * EMPTY tile: no list at all;
  * STUBBORN quadrant: 63 pixels saturate within the first chunks, one never does and keeps the quadrant's walk going to the end of the list.
check_scene() asserts those properties from the artefacts of the reference render, so the scene cannot drift away from them unnoticed."""
import numpy as np
import torch

from activesplat_amd import _lib
from activesplat_amd import rasterizer as R
from activesplat_amd import synthetic as syn
from activesplat_amd.camera import setup_camera
from tests import util

W, H = 265, 250
DENSE, EMPTY, STUBBORN = (5, 5), (12, 3), (8, 10)          # (tile column, tile row)
STUB_PIXEL = (STUBBORN[0] * 16, STUBBORN[1] * 16)           # (x, y): the corner pixel of the tile's first quadrant
T_MIN = 1e-4                                                # the blend's stop threshold

#: (mode, param) -- param 0: the mode's default; the second setting of a mode moves its thresholds to where they flip at other chunks
MODES = [(1, 0.0), (2, 0.0), (3, 0.0), (1, 0.5), (2, 1.0), (3, 1.0)]


def _tile_distance(u, v, tile):
    """Chebyshev distance in pixels of points (u, v) from the tile's pixel square"""
    x0, y0 = tile[0] * 16.0, tile[1] * 16.0
    dx = torch.clamp(torch.maximum(x0 - u, u - (x0 + 16.0)), min=0.0)
    dy = torch.clamp(torch.maximum(y0 - v, v - (y0 + 16.0)), min=0.0)
    return torch.maximum(dx, dy)


def make_scene(device):
    K = syn.intrinsics(W, H)
    fx, cx, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 2])
    g = torch.Generator().manual_seed(11)
    parts = []          # (u, v, z, sigma_px, opacity)

    # background: the benchmark's distribution, kept clear of the empty and the stubborn tile (24 pixels: more than any splat's radius)
    n = 2600
    u, v, z = torch.rand(n, generator=g) * W, torch.rand(n, generator=g) * H, 0.5 + 3.5 * torch.rand(n, generator=g)
    keep = (_tile_distance(u, v, EMPTY) > 24.0) & (_tile_distance(u, v, STUBBORN) > 24.0)
    sig = torch.exp(0.3 * torch.randn(n, generator=g)).clamp(max=2.5)
    parts.append((u[keep], v[keep], z[keep], sig[keep], torch.sigmoid(torch.randn(n, generator=g))[keep]))

    # dense tile: 320 more splats of mixed size and opacity inside one tile
    n = 320
    u = DENSE[0] * 16.0 + 16.0 * torch.rand(n, generator=g); v = DENSE[1] * 16.0 + 16.0 * torch.rand(n, generator=g)
    parts.append((u, v, 0.5 + 3.5 * torch.rand(n, generator=g), 0.5 + 2.0 * torch.rand(n, generator=g), 0.1 + 0.8 * torch.rand(n, generator=g)))

    # stubborn quadrant: four nearly opaque pixel-sized splats in front on each of 63 pixels (they stop within the first chunks), and behind
    # them 110 faint ones on the 64th, which also catches only the skirts of its three neighbours' splats
    sx, sy = STUB_PIXEL
    ys, xs = torch.meshgrid(torch.arange(8.0), torch.arange(8.0), indexing="ij")
    xs, ys = xs.reshape(-1)[1:] + sx + 0.5, ys.reshape(-1)[1:] + sy + 0.5           # (all but the corner pixel itself; a pixel's centre is at + 0.5)
    u, v = xs.repeat(4), ys.repeat(4)
    parts.append((u, v, 1.0 + 0.5 * torch.rand(u.numel(), generator=g), torch.full_like(u, 0.1), torch.full_like(u, 0.95)))
    n = 110
    parts.append((torch.full((n,), sx + 0.5), torch.full((n,), sy + 0.5), 2.0 + torch.rand(n, generator=g), torch.full((n,), 0.1),
                  torch.full((n,), 0.012)))

    u, v, z, sig, op = (torch.cat(c) for c in zip(*parts))
    P = u.numel()
    means = torch.stack([(u - cx) / fx * z, (v - cy) / fx * z, z], 1).float()
    rv = dict(means3D=means, rotations=torch.nn.functional.normalize(torch.randn(P, 4, generator=g)).float(),
              opacities=op.reshape(P, 1).float(), scales=(sig * z / fx).reshape(P, 1).repeat(1, 3).float(),
              colors_precomp=torch.rand(P, 3, generator=g).float())
    rs = setup_camera(W, H, K, np.eye(4), device=device, bg=(0.1, 0.2, 0.3))._replace(debug=True)
    return rs, {k: t.to(device) for k, t in rv.items()}


def render(rs, rv, fused):
    """One forward -> every output as a CPU tensor, final_T and n_contrib read from the image state as tests/util.py's artefacts() does"""
    P = rv["means3D"].shape[0]
    m2d = torch.zeros(P, 3, device=rv["means3D"].device)
    with torch.no_grad(), R.capture() as state:
        if fused:
            color, radii, depth, opacity, depth_sq = R.render_rgbd(rs, means2D=m2d, **rv)
        else:
            color, radii, depth, opacity = R.GaussianRasterizer(raster_settings=rs)(means2D=m2d, **rv)
            depth_sq = None
    util.LAST.clear(); util.LAST.update(state)
    art = util.artefacts()
    out = dict(color=color, depth=depth, opacity=opacity, radii=radii, final_T=torch.from_numpy(art["final_T"]),
               n_contrib=torch.from_numpy(art["n_contrib"].astype(np.int64)))
    if depth_sq is not None:
        out["depth_sq"] = depth_sq
    return {k: t.detach().cpu().clone() for k, t in out.items()}, art


def check_scene(out, art):
    gx = (W + 15) // 16
    assert gx * ((H + 15) // 16) == 272 and W % 16 and H % 16
    length = (art["ranges"][:, 1].astype(np.int64) - art["ranges"][:, 0].astype(np.int64)).reshape(-1, gx)
    fT, nc = out["final_T"].numpy(), out["n_contrib"].numpy()

    def tile(a, t):
        return a[t[1] * 16:t[1] * 16 + 16, t[0] * 16:t[0] * 16 + 16]
    assert length[EMPTY[1], EMPTY[0]] == 0 and (tile(nc, EMPTY) == 0).all() and (tile(fT, EMPTY) == 1.0).all()
    n_dense = length[DENSE[1], DENSE[0]]
    d_T, d_n = tile(fT, DENSE), tile(nc, DENSE)
    stopped = d_T < 10 * T_MIN
    assert n_dense >= 200 and stopped.sum() >= 64, (n_dense, stopped.sum())
    assert d_n[stopped].max() - d_n[stopped].min() >= 64, "the dense tile's pixels stop in different chunks"
    assert d_n[stopped].min() <= n_dense - 64, "and some of them a chunk or more before the end of the list"
    n_stub = length[STUBBORN[1], STUBBORN[0]]
    q_T, q_n = tile(fT, STUBBORN)[:8, :8].copy(), tile(nc, STUBBORN)[:8, :8].copy()
    assert n_stub >= 4 * 64
    assert q_T[0, 0] > 100 * T_MIN and q_n[0, 0] == n_stub, (q_T[0, 0], q_n[0, 0], n_stub)       # blends the list's last entry, never stopped
    q_T[0, 0], q_n[0, 0] = 0.0, 0
    assert q_T.max() < 30 * T_MIN and q_n.max() <= n_stub - 64, (q_T.max(), q_n.max(), n_stub)  # the other 63 stopped a chunk or more before


def check_bit_identical(device, fused):
    lib = _lib.get()
    rs, rv = make_scene(device)
    try:
        _lib.check(lib.gs_set_forward_priority(0, 0.0))
        ref, art = render(rs, rv, fused)
        check_scene(ref, art)
        for mode, param in MODES:
            _lib.check(lib.gs_set_forward_priority(mode, param))
            got, _ = render(rs, rv, fused)
            assert sorted(got) == sorted(ref)
            for k in ref:
                assert torch.equal(got[k], ref[k]), (mode, param, k)
    finally:
        _lib.check(lib.gs_set_forward_priority(-1, 0.0))


def check_refusals():
    lib = _lib.get()
    assert lib.gs_set_forward_priority(4, 0.0) != 0 and b"mode out of range" in lib.gs_last_error()
    assert lib.gs_set_forward_priority(1, 1.0) != 0 and b"below 1" in lib.gs_last_error()
    assert lib.gs_set_forward_priority(-1, 0.0) == 0
