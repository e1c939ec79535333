"""The textured mesh sensor at a user's shapes (GPU box): sensor.render_mesh without textures (gs_mesh_render, unchanged code) next to the same
mesh with textures (gs_mesh_render_textured: the same launches plus the texture pass), and the mip build.
  Scenes: the rooms of scripts/mesh_sensor_time.py (12 triangles; every wall cut into QUADS x QUADS quads, default 290: 1 009 200 triangles), at
  256 x 256 and 512 x 512, the same pose.  Pools: one 2048 x 2048 texture, and 64 textures of 512 x 512 (a sixty-fourth of the triangle list each),
  random texels, REPEAT.  uvs: a fixed linear map of the world position, half a tile per metre, so that a wall spans a few tiles.
  Each figure: render_mesh between its own pair of device events, CALLS (default 100) calls after 20 untimed ones, milliseconds, median and
  p10 / p90.  Every call ends in the copy of its two counters, so the device is idle when the next call begins.  "texture pass" is the difference
  of the medians.  The mip build: gs_texture_build_mips between a pair of events, 20 calls after 5 untimed ones (it rewrites the same words).
Environment: CALLS, QUADS, ONLY (a scene name).  Prints JSON."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from activesplat_amd import _lib, rasterizer as R, sensor as S, synthetic as syn  # noqa: E402
import mesh_sensor_time as base  # noqa: E402

CALLS = int(os.environ.get("CALLS", 100))
QUADS = int(os.environ.get("QUADS", 290))
ONLY = os.environ.get("ONLY", "")
POOLS = {"one_2048x2048": (1, 2048), "64_of_512x512": (64, 512)}


def textured(scene, count, size):
    rng = np.random.RandomState(1)
    v = scene.vertices.cpu().numpy().astype(np.float64)
    uvs = (v @ np.array([[1.0, 0.0], [0.0, 1.0], [0.37, 0.61]]) * 0.5).astype(np.float32)
    T = scene.num_triangles
    tri_texture = (np.arange(T, dtype=np.int64) * count // max(T, 1)).astype(np.int32)
    textures = [rng.randint(0, 256, (size, size, 3)).astype(np.uint8) for _ in range(count)]
    return S.MeshScene(scene.vertices, scene.triangles, scene.vertex_colors, device=scene.device, uvs=uvs, textures=textures, tri_texture=tri_texture)


def mip_build_ms(scene):
    lib, ms = _lib.get(), []
    for i in range(25):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.gs_texture_build_mips(scene.num_textures, scene._h_table, R._ptr(scene.texture_table), R._ptr(scene.texture_pool), scene.pool_texels,
                                             _lib.stream_ptr(scene.device)))
        b.record()
        b.synchronize()
        if i >= 5:
            ms.append(a.elapsed_time(b))
    return base.spread(ms)


def main():
    scenes = {"room_12_triangles": 1, f"room_{12 * QUADS * QUADS}_triangles": QUADS}
    out = {"render_mesh_ms": {}, "mip_build_ms": {}}
    for name, n in scenes.items():
        if ONLY and ONLY != name:
            continue
        bare = base.room(n)
        variants = {"untextured": bare}
        for pool, (count, size) in POOLS.items():
            variants[pool] = textured(bare, count, size)
            if name == "room_12_triangles":
                out["mip_build_ms"][pool] = dict(mip_build_ms(variants[pool]), pool_MB=round(variants[pool].pool_texels * 4 / 1e6, 1))
        for size in base.SIZES:
            row = {k: base.render_times(s, size, CALLS)["render_mesh_ms"] for k, s in variants.items()}
            for pool in POOLS:
                row[pool]["texture_pass_ms"] = round(row[pool]["median"] - row["untextured"]["median"], 4)
                K = syn.intrinsics(size, size, fx=size / 2.0, fy=size / 2.0)
                color, _, tri_id = S.render_mesh(variants[pool], K, base.pose(0.47, (0.3, 0.1, -0.4)), size, size)
                row[pool]["textured_pixels"] = int((tri_id >= 0).sum())
            out["render_mesh_ms"][f"{name}_{size}x{size}"] = row
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
