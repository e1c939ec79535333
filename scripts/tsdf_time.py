"""TSDF fusion and surface extraction at their own shapes (GPU box): volumes of SIZE^3 (default 128 and 256) around the bumpy room of the tests,
256 x 256 sensor frames.
  (a) gs_tsdf_integrate: one frame, and a batch of 16 frames in one sweep, between device events, `CALLS` back-to-back calls, five alternating
      repeats; next to each the bytes of the model (40 B per voxel and sweep: tsdf, weight and three colour floats read and written) over the
      time and its share of the streaming bandwidth (6.3 TB/s achievable, MI355X_MICROARCH); a run of four voxels that no frame touched is not
      written back, so the bytes really moved are 20 B per voxel read plus 20 B per voxel of the written runs: their share is reported too;
  (b) the same rule written as torch operations on the same device, one frame (what a host would write without the kernel), alternating with (a);
  (c) the ratio of one 16-frame batch to 16 single-frame sweeps;
  (d) extraction of the fused room: gs_tsdf_count (cell + point kernels and the scan) and gs_tsdf_emit (vertex + triangle kernels) between
      device events, V, T and the bytes moved (model: count reads tsdf and weight and writes two bytes per point; emit reads them back, writes a
      4-byte offset where a vertex lives, 24 B per vertex and 12 B per triangle).
The torch restatement is also compared with the kernel's volume (largest differences), so that (b) times the same arithmetic.
Environment: SIZES (default "128,256"), CALLS (default 20).  Prints JSON."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import _lib, rasterizer as R, sensor as S, volume as VOL  # noqa: E402
from tests import mesh_cases as mc  # noqa: E402

dev = torch.device("cuda")
SIZES = [int(s) for s in os.environ.get("SIZES", "128,256").split(",")]
CALLS = int(os.environ.get("CALLS", 20))
W = H = 256
STREAM_BW = 6.3e12
EXTENT = 6.6                                     # metres: the room is 4 x 2.4 x 6, the cube is centred on it


def events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_integrate(vol, points, depth, color, k4, w2c):
    """gs_tsdf_integrate's five steps for one frame as torch operations (no silhouette, no depth limit)"""
    m = torch.from_numpy(np.asarray(w2c, np.float64)[:3].astype(np.float32)).to(dev)
    c = points @ m[:, :3].T + m[:, 3]
    z = c[:, 2]
    u, v = k4[0] * c[:, 0] / z + k4[2], k4[1] * c[:, 1] / z + k4[3]
    pu, pv = torch.floor(u + 0.5), torch.floor(v + 0.5)
    ok = (z > 0) & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    pix = torch.where(ok, pv * W + pu, torch.zeros_like(pu)).long()
    d = depth.reshape(-1)[pix]
    ok &= d > 0
    sdf = d - z
    ok &= sdf >= -vol.trunc
    s = torch.clamp(sdf / vol.trunc, max=1.0)
    t, w = vol.tsdf.view(-1), vol.weight.view(-1)
    t.copy_(torch.where(ok, (t * w + s) / (w + 1), t))
    col = vol.color.view(-1, 3)
    fc = color.reshape(3, -1)[:, pix].T
    col.copy_(torch.where(ok[:, None], (col * w[:, None] + fc) / (w[:, None] + 1), col))
    w.copy_(torch.where(ok, torch.clamp(w + 1, max=vol.max_weight), w))


def main():
    room = S.MeshScene(*mc.bumpy_room(), device=dev)
    k4 = mc.k_for(W, H, 160.0)
    sensor = S.MeshSensor(room, k4, W, H)
    poses = mc.sensor_poses(16)
    depths, colors, w2cs = [], [], []
    for X in poses:
        image, depth = sensor.frame(X)
        depths.append(depth)
        colors.append((image.permute(2, 0, 1).float() / 255.0).contiguous())
        w2cs.append(sensor.w2c(X))
    depths, colors, w2cs = torch.stack(depths).contiguous(), torch.stack(colors).contiguous(), np.stack(w2cs)
    out = {"frames": [W, H], "calls": CALLS, "sizes": {}}
    lib = _lib.get()
    for n in SIZES:
        vs = EXTENT / n
        origin = (-EXTENT / 2, -EXTENT / 2, -EXTENT / 2)
        make = lambda: VOL.TsdfVolume(origin, vs, (n, n, n), 4 * vs, device=dev)          # noqa: E731
        vol = make()
        one = lambda: vol.integrate(depths[0], k4, w2cs[0], color=colors[0])               # noqa: E731
        batch = lambda: vol.integrate(depths, k4, w2cs, color=colors)                      # noqa: E731
        # the torch restatement on a volume of its own; compared once with the kernel's result for the same frame
        ref = make()
        axes = [torch.from_numpy((np.float32(origin[a]) + (np.arange(n, dtype=np.float32) + np.float32(0.5)) * np.float32(vs))).to(dev) for a in range(3)]
        gz, gy, gx = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        points = torch.stack([gx, gy, gz], -1).reshape(-1, 3).contiguous()
        k4d = [float(v) for v in k4]
        as_torch = lambda: torch_integrate(ref, points, depths[0], colors[0], k4d, w2cs[0])  # noqa: E731
        check = make()
        check.integrate(depths[0], k4, w2cs[0], color=colors[0])
        as_torch()
        written_one = float((check.weight.view(-1, 4) > 0).any(1).float().mean())           # share of the runs of four the kernel wrote back
        many = make()
        many.integrate(depths, k4, w2cs, color=colors)
        written_batch = float((many.weight.view(-1, 4) > 0).any(1).float().mean())
        del many
        same_w = float((check.weight != ref.weight).float().mean())
        agree = check.weight == ref.weight
        dt = float((check.tsdf - ref.tsdf).abs()[agree].max())
        for fn in (one, batch, as_torch):
            fn()
        torch.cuda.synchronize()
        t = {"one": [], "batch16": [], "torch_one": []}
        for _ in range(5):
            t["one"].append(events(one, CALLS)); t["batch16"].append(events(batch, max(1, CALLS // 4))); t["torch_one"].append(events(as_torch, max(1, CALLS // 4)))
        med = {k: statistics.median(v) for k, v in t.items()}
        voxels = n ** 3
        row = {"voxels": voxels, "ms": {k: [round(x, 4) for x in v] for k, v in t.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
               "model_bytes_per_sweep": 40 * voxels, "written_run_share": {"one": round(written_one, 4), "batch16": round(written_batch, 4)},
               "one_moved_TBps": round(20 * voxels * (1 + written_one) / (med["one"] * 1e-3) / 1e12, 3),
               "batch16_moved_TBps": round(20 * voxels * (1 + written_batch) / (med["batch16"] * 1e-3) / 1e12, 3),
               "one_TBps": round(40 * voxels / (med["one"] * 1e-3) / 1e12, 3), "one_share_of_6.3TBps": round(40 * voxels / (med["one"] * 1e-3) / STREAM_BW, 3),
               "batch16_TBps": round(40 * voxels / (med["batch16"] * 1e-3) / 1e12, 3), "batch16_share_of_6.3TBps": round(40 * voxels / (med["batch16"] * 1e-3) / STREAM_BW, 3),
               "batch16_over_16_singles": round(med["batch16"] / (16 * med["one"]), 3), "torch_over_kernel": round(med["torch_one"] / med["one"], 1),
               "torch_vs_kernel": {"share_of_weights_differing": same_w, "max_tsdf_difference_where_weights_agree": dt}}
        del ref, points, gx, gy, gz, check
        # extraction of the fused room
        fused = make()
        VOL.fuse_frames(fused, depths, k4, w2cs, colors=colors)
        need = int(lib.gs_tsdf_extract_scratch_bytes(n, n, n))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        st = _lib.stream_ptr(dev)
        count = lambda: _lib.check(lib.gs_tsdf_count(n, n, n, R._ptr(fused.tsdf), R._ptr(fused.weight), 1.0, R._ptr(scratch), R._ptr(counts), st))  # noqa: E731
        count()
        V, T = counts.tolist()
        vertices, vcols = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
        triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
        fp = C.POINTER(C.c_float)
        emit = lambda: _lib.check(lib.gs_tsdf_emit(n, n, n, fused.origin.ctypes.data_as(fp), fused.voxel_size, R._ptr(fused.tsdf), R._ptr(fused.color),  # noqa: E731
                                                   R._ptr(scratch), V, T, R._ptr(vertices), R._ptr(vcols), R._ptr(triangles), st))
        emit()
        torch.cuda.synchronize()
        te = {"count": [], "emit": []}
        for _ in range(5):
            te["count"].append(events(count, CALLS)); te["emit"].append(events(emit, CALLS))
        count_bytes = voxels * (4 + 4 + 2) + voxels * 2
        emit_bytes = voxels * 2 + V * (24 + 4) + T * 12
        row["extract"] = {"vertices": V, "triangles": T, "ms": {k: [round(x, 4) for x in v] for k, v in te.items()},
                          "median_ms": {k: round(statistics.median(v), 4) for k, v in te.items()}, "model_bytes": {"count": count_bytes, "emit": emit_bytes},
                          "scratch_bytes": need}
        out["sizes"][str(n)] = row
        del fused, scratch, vertices, vcols, triangles, vol
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
