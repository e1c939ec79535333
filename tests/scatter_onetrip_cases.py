"""The scatter pass of tile binning (tile_bin_kernel<true>, tilebin.hip) requests the tile counts, rects and depth bits of its whole chunk and
its cursor words in one memory round trip, whether a row is visible or not.  These cases pin what that can get wrong, against the fp32 oracle,
bit for bit, the way tests/parity_cases.py's check_forward compares the integer artefacts (tile counts, ranges, D, sorted keys and ids, radii,
n_contrib, images).  Shared by the emulated (CPU) and the GPU test file; every scene is the smallest that reaches its branch and asserts the
property it is there for from the artefacts."""
import numpy as np
import torch

from activesplat_amd import synthetic as syn
from tests import parity_cases as pc
from tests import util

CHUNK = 2048                 # kBinChunk: Gaussians per binning workgroup, in two iterations of 1024
CURSOR_TILES = 2048          # cursor words requested with the rows (two per thread): images of more tiles load the rest behind them

#: P of the size cases on a 64 x 48 image (12 tiles): a ragged first and second iteration, ragged last chunks (rows past P read row P - 1)
SIZES = [1, 1023, 1024, 1025, 2047, 2048, 2049, 2 * CHUNK + 300]


def sh_scene(N, W, H, seed, device, **kw):
    return util.scene(N, W, H, seed=seed, device=device, sh_degree=3, bg=(0.1, 0.2, 0.3), **kw)


def check_size(P, device, oracle32):
    rs, rv = sh_scene(P, 64, 48, 100 + P % 97, device)
    pc.check_forward(rs, rv, oracle32)


def check_large_rects(device, oracle32):
    """160 x 112 = 10 x 7 tiles.  Gaussian 5 covers more than 16 tiles and Gaussian 40 the whole image, both in the first wavefront next to small
    ones: that wavefront takes the balanced emitter (depth bits through LDS), the others the per-lane walk."""
    rs, rv = sh_scene(300, 160, 112, 7, device)
    sc = rv["scales"].clone()
    sc[5] = sc[5] * 12.0
    sc[40] = 3.0
    rv["scales"] = sc
    pc.check_forward(rs, rv, oracle32)
    tt = util.artefacts()["tiles_touched"]
    assert 16 < tt[5] < 70 and tt[40] == 70, (tt[5], tt[40])
    assert ((tt[:64] > 0) & (tt[:64] <= 16)).sum() >= 32 and (tt[64:] <= 16).all() and (tt[64:] > 0).any()


def check_culled_rows_over_garbage(device, oracle32):
    """A third of the Gaussians behind the camera: their rects and depth bits are never written.  The workspaces are first handed out filled with
    0x7F bytes through the caching allocator, so that what the scatter pass reads for a culled row is garbage that it must ignore."""
    P = CHUNK + 500
    rs, rv = sh_scene(P, 96, 80, 13, device)
    m = rv["means3D"].clone()
    m[::3, 2] = -m[::3, 2]
    rv["means3D"] = m
    util.run_product(rs, rv)                                  # (sizes of the workspaces of this shape)
    sizes = [int(util.LAST[k].numel() * util.LAST[k].element_size()) for k in ("geom", "image", "binning", "point_list")]
    blocks = [torch.full((n,), 0x7F, dtype=torch.uint8, device=device) for n in sizes for _ in range(2)]
    del blocks
    got, _ = pc.check_forward(rs, rv, oracle32)
    culled = got["radii"] == 0
    assert abs(int(culled[::3].sum()) - (P + 2) // 3) <= 2 and culled.sum() < 0.4 * P
    assert (util.artefacts()["tiles_touched"][culled] == 0).all()


def check_pile_on_one_tile(device, oracle32):
    """2048 pixel-sized splats of the first chunk on tile (1, 1) of a 64 x 48 image: one cursor hands out 2048 slots of one chunk, and the second
    chunk's slice of that tile starts right behind them."""
    W, H, P = 64, 48, CHUNK + 200
    rs, rv = sh_scene(P, W, H, 3, device)
    K = syn.intrinsics(W, H)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    g = torch.Generator().manual_seed(5)
    u, v, z = 19.0 + 10.0 * torch.rand(CHUNK, generator=g), 19.0 + 10.0 * torch.rand(CHUNK, generator=g), 1.0 + torch.rand(CHUNK, generator=g)
    m, sc = rv["means3D"].clone(), rv["scales"].clone()
    m[:CHUNK] = torch.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1).to(m)
    sc[:CHUNK] = (0.1 * z / fx).reshape(-1, 1).to(sc)
    rv["means3D"], rv["scales"] = m, sc
    pc.check_forward(rs, rv, oracle32)
    art = util.artefacts()
    ids = art["point_list"][art["ranges"][5, 0]:art["ranges"][5, 1]]
    assert (ids < CHUNK).sum() == CHUNK and (ids >= CHUNK).any()


def check_odd_tile_count(device, oracle32):
    """80 x 48 = 5 x 3 = 15 tiles"""
    rs, rv = sh_scene(700, 80, 48, 21, device)
    pc.check_forward(rs, rv, oracle32)


def check_more_tiles_than_cursor_rounds(device, oracle32):
    """17 x 16400 pixels = 2 x 1025 = 2050 tiles: two more cursor words than a thread requests with its rows -- the tail loop behind them"""
    W, H = 17, 16400
    assert ((W + 15) // 16) * ((H + 15) // 16) == CURSOR_TILES + 2
    rs, rv = sh_scene(1500, W, H, 17, device)
    pc.check_forward(rs, rv, oracle32)
    rg = util.artefacts()["ranges"]
    assert (rg[CURSOR_TILES:, 1] > rg[CURSOR_TILES:, 0]).any(), "the tiles behind the requested cursor words are empty"


def check_cov3d_precomp(device, oracle32):
    from oracle.dense_torch import build_cov3d
    rs, rv = sh_scene(CHUNK + 77, 64, 48, 31, device)
    S = build_cov3d(rv["scales"].cpu(), rv["rotations"].cpu(), 1.0)
    rv["cov3D_precomp"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float().to(device)
    rv.pop("scales"); rv.pop("rotations")
    pc.check_forward(rs, rv, oracle32)


def check_backward(device, oracle64, oracle32):
    """The tile lists are what the backward walks: its gradients against the fp64 oracle on a two-chunk scene with culled rows"""
    rs, rv = sh_scene(CHUNK + 150, 64, 48, 41, device)
    m = rv["means3D"].clone()
    m[::4, 2] = -m[::4, 2]
    rv["means3D"] = m
    pc.check_backward(rs, rv, oracle64, oracle32=oracle32)
