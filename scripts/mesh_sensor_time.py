"""The mesh RGB-D sensor at a user's shapes (GPU box): sensor.render_mesh and SplatMapper.run_sensor.
  (1) sensor.render_mesh between its own pair of device events at SIZES (256 x 256 and 512 x 512) on the 12-triangle room and on the same room with
      every wall tessellated into QUADS x QUADS quads (default 290: 1 009 200 triangles); CALLS (default 100) calls after 20 untimed ones;
      milliseconds, median and p10 / p90.  Every call ends in the copy of its two counters, so the device is idle when the next call begins: the
      figure holds the four launches, their enqueue gaps and the scratch allocation, not the kernels alone -- those come from
      `rocprofv3 --kernel-trace --stats -- python scripts/mesh_sensor_time.py` with PROFILE=1 (20 calls per set-up, nothing else) and
      ONLY=<set-up name> (one set-up per profiler run, so that the per-kernel averages belong to one shape).
      With each set-up: D (the length of the tile lists) and the longest tile list.
  (2) host wall time of one SplatMapper.run_sensor frame next to one run_raw frame of the same size (the frame rendered beforehand and copied to
      the host), FRAMES (default 12) poses stepping through the room, device_ingest on, a synchronise behind every frame; frame 0 left out;
      milliseconds, median and [min - max].  Left out when PROFILE or ONLY is set.
Environment: CALLS, QUADS, FRAMES, PROFILE, ONLY.  Prints JSON."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from activesplat_amd import frames as FR, sensor as S, synthetic as syn  # noqa: E402
from activesplat_amd.mapper import SplatMapper  # noqa: E402

dev = torch.device("cuda")
CALLS = int(os.environ.get("CALLS", 100))
QUADS = int(os.environ.get("QUADS", 290))
FRAMES = int(os.environ.get("FRAMES", 12))
PROFILE = os.environ.get("PROFILE", "0") == "1"
ONLY = os.environ.get("ONLY", "")
SIZES = (256, 512)
ROOM = ((-2.0, 2.0), (-1.2, 1.2), (-3.0, 3.0))


def room(n):
    """the room box with every wall cut into n x n quads (two triangles each); lattice vertices shared, random vertex colours"""
    index, verts, tris = {}, [], []

    def vid(ijk):
        if ijk not in index:
            index[ijk] = len(verts)
            verts.append([ROOM[a][0] + (ROOM[a][1] - ROOM[a][0]) * ijk[a] / n for a in range(3)])
        return index[ijk]
    for axis in range(3):
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    q = []
                    for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        ijk = [0, 0, 0]
                        ijk[axis], ijk[(axis + 1) % 3], ijk[(axis + 2) % 3] = side, a + da, b + db
                        q.append(vid(tuple(ijk)))
                    tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    v = np.array(verts, np.float32)
    colors = np.random.RandomState(0).randint(0, 256, (len(v), 3)).astype(np.uint8)
    return S.MeshScene(v, np.array(tris, np.int32), colors, device=dev)


def pose(yaw, position):
    """world-to-camera of a camera at `position` turned by `yaw` about the vertical (x right, y down, z forward)"""
    c, s = np.cos(yaw), np.sin(yaw)
    c2w = np.eye(4)
    c2w[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    c2w[:3, 3] = position
    return np.linalg.inv(c2w)


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "p10": round(v[len(v) // 10], 4), "p90": round(v[(9 * len(v)) // 10], 4)}


def render_times(scene, size, calls):
    K = syn.intrinsics(size, size, fx=size / 2.0, fy=size / 2.0)
    w2c = pose(0.47, (0.3, 0.1, -0.4))
    ms = []
    for i in range(20 + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        S.render_mesh(scene, K, w2c, size, size)
        b.record()
        b.synchronize()
        if i >= 20:
            ms.append(a.elapsed_time(b))
    return {"render_mesh_ms": spread(ms), "D": scene.last_counts[0], "longest_tile_list": scene.last_counts[1]}


def sensor_poses(n):
    out, position, yaw = [], np.array([0.0, 0.0, 1.5]), 0.0
    for _ in range(n):
        c, s = np.cos(yaw), np.sin(yaw)
        X = np.eye(4)
        X[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        X[:3, 3] = position
        out.append(X)
        position = position + 0.1 * (X[:3, :3] @ np.array([0.0, 0.0, -1.0]))
        yaw += np.deg2rad(10.0)
    return out


def quat(rot):
    w = np.sqrt(max(0.0, 1.0 + rot[0, 0] + rot[1, 1] + rot[2, 2])) / 2
    return np.array([w, (rot[2, 1] - rot[1, 2]) / (4 * w), (rot[0, 2] - rot[2, 0]) / (4 * w), (rot[1, 0] - rot[0, 1]) / (4 * w)], np.float32)


def frame_times(scene, size, through_host):
    K = syn.intrinsics(size, size, fx=size / 2.0, fy=size / 2.0)
    sensor = S.MeshSensor(scene, K, size, size)
    poses = sensor_poses(FRAMES)
    mp = SplatMapper(K, size, size, config=dict(step_num=FRAMES, densify_downscale_factor=2, device_ingest=True), device=dev)
    first, ms = None, []
    for fid, X in enumerate(poses):
        gt, first = FR.gt_w2c_from_pose(X, first)
        q, t = quat(gt[:3, :3].astype(np.float64)), gt[:3, 3]
        if through_host:
            image, depth = (a.cpu().numpy() for a in sensor.frame(X))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if through_host:
            mp.run_raw(image, depth, X, fid, q, t)
        else:
            mp.run_sensor(sensor, X, fid, q, t)
        torch.cuda.synchronize()
        if fid > 0:
            ms.append(1e3 * (time.perf_counter() - t0))
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    scenes = {"room_12_triangles": 1, f"room_{12 * QUADS * QUADS}_triangles": QUADS}
    scenes = {name: room(n) for name, n in scenes.items() if not ONLY or ONLY.startswith(name)}
    out = {"render_mesh": {}}
    for name, scene in scenes.items():
        for size in SIZES:
            if not ONLY or ONLY == f"{name}_{size}x{size}":
                out["render_mesh"][f"{name}_{size}x{size}"] = render_times(scene, size, 20 if PROFILE else CALLS)
    if not PROFILE and not ONLY:
        small = scenes["room_12_triangles"]
        out["frame_host_ms_256x256"] = {"run_sensor": frame_times(small, 256, False), "run_raw": frame_times(small, 256, True),
                                        "run_sensor_again": frame_times(small, 256, False), "run_raw_again": frame_times(small, 256, True)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
